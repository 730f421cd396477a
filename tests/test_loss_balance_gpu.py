"""hn_balanced_sum and hn_balance_hold (csrc/hn_loss.hip) through the C entry points, over the kernel's whole range: n in
{1, 3, 5, 6, 8} terms in one group, three groups, groups of one; losses from 1e-6 to 1e4 and exact zeros; log-variances inside the clamp,
at +-S, outside it, and NaN in slots no term owns.  Every output lies between guard bands.

Bounds and where they come from
  total, seeds, ds, activity, record        ==  form (a) of tests/loss_balance_ref.py, given the e_i read back from the record
  e_i against exp(-s~_i) in float64          rtol 2e-6: what the project gives the device's expf (test_post_gpu.py::_check_lanes)
  at s = 0: total and seeds                  ==  hn_weighted_sum's on the same inputs
  slots of s no term owns, s itself          untouched (bit patterns compared)
An inactive term (loss exactly 0) has ds and activity exactly 0.0; its loss seed is the formula's ((gout * gw) * w) * e, which at s = 0 is
hn_weighted_sum's seed -- the two cannot both be asked of a zero loss, and the s = 0 identity is the one the formulas state."""
import ctypes

import numpy as np
import pytest
import torch

from tests import loss_balance_ref as R
from tests.guards import Guarded, dev

pytestmark = pytest.mark.gpu

F = np.float32
S = 6.0
NAN_BITS = 0x7FC00123


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    import __graft_entry__ as g
    g.build()
    from multitask_hydranet_amd._lib import lib
    return lib()


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


GROUPINGS = {1: ([0], [0]), 3: ([0, 0, 0], [0, 1, 2]), 5: ([0] * 5, [0, 1, 1, 1, 2]), 6: ([0] * 6, [0, 1, 1, 2, 2, 2]),
             8: ([0] * 8, [0, 0, 0, 1, 2, 2, 2, 2])}          # n -> (one group, three groups with a group of one) -- n = 1: one group twice


def case(n, grouping, seed, kind):
    """kind: 'inside' | 'edges' (s at +-S and outside +-S among inside values) | 'zero' (s = 0).  Every case has exact zeros among the
    losses (n > 1) and spans 1e-6 .. 1e4; slots no term owns hold a NaN pattern."""
    rng = np.random.default_rng(seed)
    x = (10.0 ** np.linspace(-6, 4, n)).astype(F)
    rng.shuffle(x)
    if n > 1:
        x[int(rng.integers(0, n))] = 0
    if n >= 6:
        x[n - 1] = 0
    w = rng.uniform(0.5, 50.0, n).astype(F)
    grp = GROUPINGS[n][grouping]
    gw = rng.uniform(0.5, 2.0, max(grp) + 1).astype(F)
    n_slots = 8 if n > 6 else 6
    slot = sorted(rng.choice(n_slots, n, replace=False).tolist())
    s = np.frombuffer(np.full(n_slots, NAN_BITS, np.uint32).tobytes(), F).copy()
    if kind == "zero":
        vals = np.zeros(n, F)
    else:
        vals = rng.uniform(-5.0, 5.0, n).astype(F)
        if kind == "edges":
            for i, v in zip(rng.permutation(n), (S, -S, 2 * S, -2 * S, np.nextafter(F(S), F(0)), -7.5)):
                vals[i] = v
    s[slot] = vals
    return x, w, grp, gw, slot, s, n_slots


class Call:
    """device-side arguments of one hn_balanced_sum case; outputs between guard bands, s in a guarded buffer of its own"""

    def __init__(self, lib, x, w, grp, gw, slot, s, n_slots, gout):
        self.lib, self.n, self.ns = lib, len(x), n_slots
        self.xd = torch.from_numpy(np.asarray(x, F)).to(dev())
        self.ptrs = (ctypes.c_void_p * self.n)(*[self.xd.data_ptr() + 4 * i for i in range(self.n)])
        self.wa = (ctypes.c_float * self.n)(*[float(v) for v in w])
        self.ga = (ctypes.c_float * len(gw))(*[float(v) for v in gw])
        self.ia = (ctypes.c_int * self.n)(*[int(v) for v in grp])
        self.sa = (ctypes.c_int * self.n)(*[int(v) for v in slot])
        self.s = Guarded(1, n_slots)
        self.s.view.copy_(torch.from_numpy(np.asarray(s, F)).view(1, -1))
        self.g = torch.tensor([gout], dtype=torch.float32, device=dev())
        self.out, self.rec, self.grads, self.ds = Guarded(1, 1), Guarded(1, 16), Guarded(1, self.n), Guarded(1, 2 * n_slots)

    def _call(self, fwd, bwd):
        self.lib.call("hn_balanced_sum", ctypes.addressof(self.ptrs), ctypes.addressof(self.wa), ctypes.addressof(self.ga),
                      ctypes.addressof(self.ia), ctypes.addressof(self.sa), self.n, self.ns, self.s.ptr(), S,
                      self.g.data_ptr() if bwd else None, self.out.ptr() if fwd else None, self.rec.ptr(),
                      self.grads.ptr() if bwd else None, self.ds.ptr() if bwd else None)

    def forward(self):
        self._call(True, False)

    def backward(self):
        self._call(False, True)

    def read(self):
        get = lambda gd: gd.view.cpu().numpy()[0].copy()
        res = dict(out=get(self.out)[0], rec=get(self.rec), grads=get(self.grads), ds=get(self.ds), s=get(self.s))
        for name in ("out", "rec", "grads", "ds", "s"):
            getattr(self, name).check(name)
        return res


def check_against_ref(got, x, w, grp, gw, slot, s, n_slots, gout):
    n = len(x)
    e = got["rec"][:n]
    e64 = np.exp(-R.clamp_s(np.asarray(s, np.float64)[slot], S, np.float64))
    print("e", e, "exp", e64, "total", got["out"], "ds", got["ds"])
    np.testing.assert_allclose(e.astype(np.float64), e64, rtol=2e-6, atol=0)
    tot, act = R.exact_forward(x, w, grp, gw, slot, s, S, e)
    seeds, ds = R.exact_backward(x, w, grp, gw, slot, s, S, e, F(gout), n_slots)
    assert bits(got["out"]) == bits(tot), (got["out"], tot)
    assert (bits(got["rec"][8:8 + n]) == bits(act.astype(F))).all()
    assert (bits(got["rec"][n:8]) == 0).all() and (bits(got["rec"][8 + n:]) == 0).all()          # unused entries: 0.0, not stale
    assert (bits(got["grads"]) == bits(seeds)).all(), (got["grads"], seeds)
    assert (bits(got["ds"]) == bits(ds)).all(), (got["ds"], ds)
    # inactive terms and slots no term owns: ds and activity exactly 0.0; s untouched everywhere
    owned = {k: i for i, k in enumerate(slot)}
    for k in range(n_slots):
        if k not in owned or x[owned[k]] == 0:
            assert bits(got["ds"][k]) == 0 and bits(got["ds"][n_slots + k]) == 0
    assert (bits(got["s"]) == bits(s)).all()


@pytest.mark.parametrize("kind", ["inside", "edges"])
@pytest.mark.parametrize("grouping", [0, 1])
@pytest.mark.parametrize("n", [1, 3, 5, 6, 8])
def test_balanced_sum_is_the_exact_form(lib, n, grouping, kind):
    x, w, grp, gw, slot, s, ns = case(n, grouping, 100 * n + grouping, kind)
    c = Call(lib, x, w, grp, gw, slot, s, ns, gout=1.7)
    c.forward()
    c.backward()
    first = c.read()
    check_against_ref(first, x, w, grp, gw, slot, s, ns, 1.7)
    c2 = Call(lib, x, w, grp, gw, slot, s, ns, gout=1.7)        # a second run, fresh buffers: the same bits
    c2.forward()
    c2.backward()
    second = c2.read()
    for k in first:
        assert (bits(first[k]) == bits(second[k])).all(), k


@pytest.mark.parametrize("grouping", [0, 1])
@pytest.mark.parametrize("n", [1, 3, 5, 6, 8])
def test_zero_log_variances_are_the_weighted_sum(lib, n, grouping):
    x, w, grp, gw, slot, s, ns = case(n, grouping, 7 * n + grouping, "zero")
    c = Call(lib, x, w, grp, gw, slot, s, ns, gout=0.37)
    c.forward()
    c.backward()
    got = c.read()
    g = torch.tensor([0.37], dtype=torch.float32, device=dev())
    out, grads = Guarded(1, 1), Guarded(1, n)
    lib.call("hn_weighted_sum", ctypes.addressof(c.ptrs), ctypes.addressof(c.wa), ctypes.addressof(c.ga), ctypes.addressof(c.ia), n,
             g.data_ptr(), out.ptr(), grads.ptr())
    want_out, want_grads = out.view.cpu().numpy()[0, 0], grads.view.cpu().numpy()[0]
    assert (bits(got["rec"][:n]) == bits(np.ones(n, F))).all()                  # expf(-0) is exactly 1
    assert bits(got["out"]) == bits(want_out), (got["out"], want_out)
    assert (bits(got["grads"]) == bits(want_grads)).all(), (got["grads"], want_grads)
    check_against_ref(got, x, w, grp, gw, slot, s, ns, 0.37)


def test_single_call_does_forward_and_backward(lib):
    x, w, grp, gw, slot, s, ns = case(6, 1, 3, "edges")
    a, b = Call(lib, x, w, grp, gw, slot, s, ns, 2.0), Call(lib, x, w, grp, gw, slot, s, ns, 2.0)
    a.forward()
    a.backward()
    b._call(True, True)
    ra, rb = a.read(), b.read()
    for k in ra:
        assert (bits(ra[k]) == bits(rb[k])).all(), k


def test_replay_in_a_captured_graph_sees_the_new_log_variances(lib):
    x, w, grp, gw, slot, s, ns = case(6, 1, 11, "inside")
    c = Call(lib, x, w, grp, gw, slot, s, ns, gout=1.0)
    c.forward()
    c.backward()                                         # (warm: nothing is loaded for the first time inside the capture)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        c.forward()
        c.backward()
    graph.replay()
    check_against_ref(c.read(), x, w, grp, gw, slot, s, ns, 1.0)
    s2 = s.copy()
    s2[slot] = np.linspace(-7.0, 7.0, len(slot)).astype(F)                    # changed in place, the clamp's outside included
    c.s.view.copy_(torch.from_numpy(s2).view(1, -1))
    x2 = x.copy()
    x2[0], x2[1] = 0.0, 3.0
    c.xd.copy_(torch.from_numpy(x2))
    graph.replay()
    check_against_ref(c.read(), x2, w, grp, gw, slot, s2, ns, 1.0)


def test_argument_checks(lib):
    from multitask_hydranet_amd._lib import HipKernelError
    x, w, grp, gw, slot, s, ns = case(5, 1, 1, "inside")
    for kw in (dict(slot=slot[::-1]), dict(slot=[0, 1, 2, 3, 6]), dict(grp=grp[::-1])):
        a = dict(x=x, w=w, grp=grp, gw=gw, slot=slot, s=s, n_slots=ns, gout=1.0)
        a.update(kw)
        c = Call(lib, **a)
        with pytest.raises(HipKernelError):
            c.forward()
        assert not torch.isfinite(c.out.view).any()      # nothing was written
    c = Call(lib, x, w, grp, gw, slot, s, ns, 1.0)
    c.ns = 4                                             # fewer slots than terms
    with pytest.raises(HipKernelError):
        c.forward()
    torch.cuda.synchronize()


def test_hold_gives_inactive_slots_back(lib):
    n = 6
    rng = np.random.default_rng(0)
    old = [rng.normal(size=n).astype(F) for _ in range(3)]
    new = [rng.normal(size=n).astype(F) for _ in range(3)]
    act = np.array([1.0, 0.0, 0.5, 0.0, 1.0, 0.0], F)            # (0.5: active in one of two accumulated micro-batches)
    t = [Guarded(1, n) for _ in range(3)]
    hold = Guarded(1, 3 * n)
    for g, o in zip(t, old):
        g.view.copy_(torch.from_numpy(o).view(1, -1))
    lib.call("hn_balance_hold", t[0].ptr(), t[1].ptr(), t[2].ptr(), hold.ptr(), None, n)
    assert (bits(hold.view.cpu().numpy()[0]) == bits(np.concatenate(old))).all()
    for g, v in zip(t, new):                                       # what an Adam step would leave
        g.view.copy_(torch.from_numpy(v).view(1, -1))
    ad = torch.from_numpy(act).to(dev())
    lib.call("hn_balance_hold", t[0].ptr(), t[1].ptr(), t[2].ptr(), hold.ptr(), ad.data_ptr(), n)
    for g, o, v, name in zip(t, old, new, "smv"):
        assert (bits(g.view.cpu().numpy()[0]) == bits(np.where(act > 0, v, o))).all(), name
        g.check(name)
    hold.check("hold")
