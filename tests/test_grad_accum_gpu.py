"""Gradient accumulation on the device: hn_grad_accum against the numpy yardstick (tests/grad_accum_ref.py), bit for bit, on tables built
here from the header's description; then optim.GradAccumulator + optim.Adam.step(grads=) against a second Adam whose p.grad was set to
the yardstick's mean."""
import ctypes

import numpy as np
import pytest
import torch

from tests import grad_accum_ref as ref

pytestmark = pytest.mark.gpu

SIZES = [1, 3, 4, 5, 1023, 1024, 1025, 4099]
SENTINEL = 0x7FC12345                                     # a NaN with a payload: what the kernel must not write, read or move


@pytest.fixture(scope="module")
def built():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    import __graft_entry__ as g
    g.build()
    from multitask_hydranet_amd._lib import lib
    return lib()


def dev():
    return torch.device("cuda:0")


def bits(t):
    return t.detach().contiguous().view(torch.int32).cpu().numpy().reshape(-1)


class Arena:
    """the launch's tensors in two flat buffers.  g: every size twice -- 16-byte aligned, and one element further (misaligned against
    its accumulator slot) -- with sentinel words around each; acc: one 16-byte-aligned slot per job, sentinel padding between the slots"""

    def __init__(self, sizes=SIZES):
        self.jobs = []                                    # (g offset, acc offset, numel)
        goff, aoff = 0, 4
        for shift in (0, 1):
            for n in sizes:
                self.jobs.append((goff + 4 + shift, aoff, n))
                goff += (n + 12 + 3) // 4 * 4
                aoff += (n + 3) // 4 * 4 + 4
        self.g_host = np.full(goff, SENTINEL, dtype=np.int32)
        self.a_host = np.full(aoff, SENTINEL, dtype=np.int32)
        self.g = torch.from_numpy(self.g_host.copy()).to(dev())
        self.a = torch.from_numpy(self.a_host.copy()).to(dev())
        assert self.g.data_ptr() % 16 == 0 and self.a.data_ptr() % 16 == 0
        rows, owner, blk = [], [], 0
        for i, (go, ao, n) in enumerate(self.jobs):
            nb = (n + 1023) // 1024
            rows.append([self.g.data_ptr() + 4 * go, self.a.data_ptr() + 4 * ao, n, blk])
            owner += [i] * nb
            blk += nb
        assert {r[0] % 16 for r in rows} == {0, 4} and {r[1] % 16 for r in rows} == {0}
        self.table = torch.tensor(rows, dtype=torch.int64).to(dev())
        self.owner = torch.tensor(owner, dtype=torch.int32).to(dev())
        self.blocks = blk

    def set_g(self, arrays):
        """arrays: one int32 word array per job"""
        for (go, _, n), x in zip(self.jobs, arrays):
            self.g_host[go:go + n] = x
        self.g.copy_(torch.from_numpy(self.g_host))

    def launch(self, l, j, losses=(), means=None, words=(), sticky=None):
        la = (ctypes.c_void_p * max(len(losses), 1))(*[t.data_ptr() for t in losses])
        wa = (ctypes.c_void_p * max(len(words), 1))(*[t.data_ptr() for t in words])
        l.call("hn_grad_accum", self.table.data_ptr(), self.owner.data_ptr(), self.blocks, j, ctypes.addressof(la) if losses else None,
               len(losses), None if means is None else means.data_ptr(), ctypes.addressof(wa) if words else None, len(words),
               None if sticky is None else sticky.data_ptr())

    def expect(self, arrays):
        """the yardstick's accumulators written into the host image of the acc buffer"""
        for (_, ao, n), x in zip(self.jobs, arrays):
            self.a_host[ao:ao + n] = x

    def check(self, what):
        torch.cuda.synchronize()
        assert np.array_equal(bits(self.g), self.g_host), (what, "g or the words around it changed")
        got = bits(self.a)
        bad = np.nonzero(got != self.a_host)[0]
        assert bad.size == 0, (what, bad[:8], got[bad[:8]], self.a_host[bad[:8]])


def floats(gen, n, scale=1.0):
    return (gen.standard_normal(n) * scale).astype(np.float32)


def test_sizes_and_alignment_against_the_yardstick(built):
    """every size twice with the same values: g 16-byte aligned, and g one element further; j = 1, 2, 3, 7 in sequence"""
    ar = Arena()
    gen = np.random.default_rng(1)
    acc = [None] * len(ar.jobs)
    for j in (1, 2, 3, 7):
        gs = [floats(gen, n, 10.0 ** (i % 5 - 2)) for i, n in enumerate(SIZES)] * 2
        ar.set_g([x.view(np.int32) for x in gs])
        ar.launch(built, j)
        acc = [ref.accumulate(a, x, j) for a, x in zip(acc, gs)]
        ar.expect([a.view(np.int32) for a in acc])
        ar.check(j)                                                                # the accumulators, their padding, g and the words around it
    got = bits(ar.a)
    for (_, a0, n), (_, a1, _) in zip(ar.jobs[:len(SIZES)], ar.jobs[len(SIZES):]):
        assert np.array_equal(got[a0:a0 + n], got[a1:a1 + n]), n                   # the bits do not depend on the alignment


def test_first_micro_batch_does_not_read_the_accumulator(built):
    """the accumulator holds NaN bit patterns; g holds arbitrary words (-0, denormals, infinities, NaNs of many payloads among them)"""
    ar = Arena()
    gen = np.random.default_rng(2)
    ar.a.copy_(torch.from_numpy(np.full(ar.a_host.size, 0x7FFFFFFF, dtype=np.int32)))
    ar.a_host[:] = 0x7FFFFFFF
    gs = []
    for _, _, n in ar.jobs:
        w = gen.integers(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32).view(np.int32)
        special = np.array([0x80000000, 0x00000001, 0x807FFFFF, 0x7FC00001, 0xFFC12345, 0x7F800001, 0x7F800000, 0xFF800000], dtype=np.uint32)
        w[:min(n, 8)] = special.view(np.int32)[:min(n, 8)]
        gs.append(w)
    ar.set_g(gs)
    ar.launch(built, 1)
    ar.expect(gs)
    ar.check("j == 1")


def test_non_finite_gradients_stay_where_they_are(built):
    ar = Arena()
    gen = np.random.default_rng(3)
    plant = {4: (1023 - 1, np.nan), 6: (1024, np.inf), 7: (4098, -np.inf), 8: (0, np.nan), 15: (2049, np.inf)}    # job -> (element, value)
    acc = [None] * len(ar.jobs)
    for j in (1, 2, 3):
        gs = [floats(gen, n) for _, _, n in ar.jobs]
        if j == 2:
            for job, (e, v) in plant.items():
                gs[job][e] = v
        ar.set_g([x.view(np.int32) for x in gs])
        ar.launch(built, j)
        acc = [ref.accumulate(a, x, j) for a, x in zip(acc, gs)]
    torch.cuda.synchronize()
    got = bits(ar.a)
    for i, ((_, ao, n), want) in enumerate(zip(ar.jobs, acc)):
        out = got[ao:ao + n].view(np.float32)
        keep = np.ones(n, dtype=bool)
        if i in plant:
            keep[plant[i][0]] = False
            assert not np.isfinite(out[plant[i][0]]) and not np.isfinite(want[plant[i][0]]), i
        assert np.isfinite(out[keep]).all(), i
        assert np.array_equal(out[keep].view(np.int32), want[keep].view(np.int32)), i


@pytest.mark.parametrize("n_losses", [1, 3, 8])
def test_loss_means_and_sticky_word(built, n_losses):
    ar = Arena(sizes=[5, 1025])
    gen = np.random.default_rng(10 + n_losses)
    losses = [torch.zeros((), device=dev()) for _ in range(n_losses)]
    words = [torch.zeros((1,), dtype=torch.int32, device=dev()) for _ in range(2)]
    means = torch.from_numpy(np.full(8, SENTINEL, dtype=np.int32)).to(dev())
    sticky = torch.full((1,), 0x55, dtype=torch.int32, device=dev())
    nan = float("nan")
    # (j, index of a NaN loss or None, raised word or None): three groups -- all clean; a NaN loss at micro-batch 2 that sticks; a word
    # raised at micro-batch 1 and clear again at 2 -- each starting at j == 1 after what the group before left
    plan = [(1, None, None), (2, None, None), (3, None, None),
            (1, None, None), (2, n_losses - 1, None), (3, None, None),
            (1, None, 1), (2, None, None),
            (1, None, None)]
    want_sticky = [0, 0, 0, 0, 2, 2, 4, 4, 0]
    mean, prev, dirty = None, 0x55, None
    ar.set_g([floats(gen, n).view(np.int32) for _, _, n in ar.jobs])
    for (j, bad, word), ws in zip(plan, want_sticky):
        vals = floats(gen, n_losses, 3.0)
        if bad is not None:
            vals[bad] = nan
        for t, v in zip(losses, vals):
            t.fill_(float(v))
        wv = [0, 0]
        if word is not None:
            wv[word] = 7
        for t, v in zip(words, wv):
            t.fill_(v)
        ar.launch(built, j, losses, means.view(torch.float32), words, sticky)
        torch.cuda.synchronize()
        mean = ref.accumulate(mean, vals, j)
        prev = ref.sticky(prev, j, vals, wv)
        if j == 1:
            dirty = None
        if bad is not None:
            dirty = bad
        assert prev == ws and int(sticky.item()) == ws, (j, bad, word, int(sticky.item()))
        got = bits(means)
        keep = np.arange(n_losses) != (-1 if dirty is None else dirty)
        assert np.array_equal(got[:n_losses][keep], mean.view(np.int32)[keep]), (j, got, mean)
        if dirty is not None:
            assert not np.isfinite(got[:n_losses].view(np.float32)[dirty])
        assert (got[n_losses:] == SENTINEL).all()                                  # the means past n_losses are not written


def test_no_losses_and_no_words_with_null_pointers(built):
    ar = Arena(sizes=[3, 1025])
    gen = np.random.default_rng(4)
    acc = [None] * len(ar.jobs)
    for j in (1, 2):
        gs = [floats(gen, n) for _, _, n in ar.jobs]
        ar.set_g([x.view(np.int32) for x in gs])
        ar.launch(built, j)                                                        # losses, loss_mean, words, sticky: all NULL
        acc = [ref.accumulate(a, x, j) for a, x in zip(acc, gs)]
        ar.expect([a.view(np.int32) for a in acc])
        ar.check(j)


def test_capturable(built):
    """one launch recorded in a hipGraph and replayed twice (j fixed at 2) equals two eager launches"""
    gen = np.random.default_rng(5)
    eager, graphed = Arena(sizes=[5, 1023, 4099]), Arena(sizes=[5, 1023, 4099])
    gs = [floats(gen, n) for _, _, n in eager.jobs]
    start = [floats(gen, n) for _, _, n in eager.jobs]
    loss = torch.full((), 1.5, device=dev())
    for ar in (eager, graphed):
        ar.set_g([x.view(np.int32) for x in gs])
        ar.expect([x.view(np.int32) for x in start])
        ar.a.copy_(torch.from_numpy(ar.a_host))
        ar.means = torch.tensor([4.0] + [0.0] * 7, device=dev())
        ar.sticky = torch.zeros((1,), dtype=torch.int32, device=dev())
    for _ in range(2):
        eager.launch(built, 2, [loss], eager.means, [], eager.sticky)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        graphed.launch(built, 2, [loss], graphed.means, [], graphed.sticky)
    torch.cuda.synchronize()
    assert np.array_equal(bits(graphed.a), graphed.a_host)                         # a capture runs nothing
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    acc = [ref.accumulate(ref.accumulate(a, x, 2), x, 2) for a, x in zip(start, gs)]
    eager.expect([a.view(np.int32) for a in acc])
    eager.check("eager")
    assert np.array_equal(bits(graphed.a), bits(eager.a))
    assert np.array_equal(bits(graphed.means), bits(eager.means)) and float(eager.means[0]) == 2.125
    assert int(graphed.sticky.item()) == 0 == int(eager.sticky.item())


# ------------------------------------------------------------------------------------------------------------------------------------
SHAPES = [(7,), (3, 5), (1,), (64, 8, 3, 3), (1023,), (1025,), (2, 2)]             # the last one never gets a gradient


def state_bits(opt, ps, ema):
    out = []
    for p in ps:
        st = opt.state.get(p, {})
        out.append([bits(p)] + [bits(st[k]) for k in ("exp_avg", "exp_avg_sq") + (("ema",) if ema else ()) if k in st])
    return out


def same_state(a, b):
    return all(len(x) == len(y) and all(np.array_equal(u, v) for u, v in zip(x, y)) for x, y in zip(a, b))


@pytest.mark.parametrize("variant", ["plain", "clip", "ema"])
def test_step_with_grads_uses_the_mean_and_leaves_p_grad_alone(built, variant):
    from multitask_hydranet_amd.optim import Adam, GradAccumulator
    keys = dict(plain={}, clip=dict(max_grad_norm=0.5, skip_nonfinite=True), ema=dict(skip_nonfinite=True, ema_decay=0.9))[variant]
    gen = torch.Generator().manual_seed(11)
    init = [torch.randn(s, generator=gen).to(dev()) for s in SHAPES]
    pa = [torch.nn.Parameter(p.clone()) for p in init]
    pb = [torch.nn.Parameter(p.clone()) for p in init]
    oa, ob = Adam(pa, 1e-2, weight_decay=1e-2, **keys), Adam(pb, 1e-2, weight_decay=1e-2, **keys)
    acc = GradAccumulator(pa)
    assert acc.pending == 0 and all(acc.flat[o:].data_ptr() % 16 == 0 for o in acc.offsets)
    loss = torch.ones((), device=dev())
    for group in range(3):                                                         # (the third group runs Adam's cached tables)
        seen = []
        for j in range(3):
            gs = [torch.randn(s, generator=gen) * 10.0 ** (i - 3) for i, s in enumerate(SHAPES[:-1])]
            seen.append(gs)
            for p, g in zip(pa, gs):
                p.grad = g.to(dev())
            acc.add(losses=[loss])
            assert acc.pending == j + 1
        held = [(p.grad, bits(p.grad)) for p in pa[:-1]]
        for i, p in enumerate(pa[:-1]):
            want = ref.mean_of([s[i].numpy() for s in seen])
            assert np.array_equal(bits(acc.grad(p)), want.view(np.int32).reshape(-1)) and acc.grad(p).shape == p.shape
            pb[i].grad = torch.from_numpy(want).to(dev())
        assert acc.grad(pa[-1]) is None
        if keys:
            oa.step(grads=acc, losses=[acc.loss_means()[0]], guard_words=[acc.sticky_word])
            ob.step(losses=[loss])
        else:
            oa.step(grads=acc)
            ob.step()
        acc.reset()
        assert acc.pending == 0
        for p, (g, b) in zip(pa[:-1], held):
            assert p.grad is g and np.array_equal(bits(p.grad), b)                 # neither rebound nor written
        assert pa[-1].grad is None and pa[-1] not in oa.state
        assert same_state(state_bits(oa, pa, "ema_decay" in keys), state_bits(ob, pb, "ema_decay" in keys)), (variant, group)
        assert not np.array_equal(bits(pa[0]), bits(init[0]))
    if keys:
        ra, rb = oa.grad_guard_record(), ob.grad_guard_record()
        assert ra == rb and ra["steps"] == 3 and ra["skipped"] == 0, (ra, rb)
        assert variant != "clip" or ra["coef"] < 1.0


def test_sticky_word_skips_the_step(built):
    from multitask_hydranet_amd.optim import Adam, GradAccumulator
    gen = torch.Generator().manual_seed(12)
    ps = [torch.nn.Parameter(torch.randn(s, generator=gen).to(dev())) for s in SHAPES[:-1]]
    opt = Adam(ps, 1e-2, weight_decay=1e-2, skip_nonfinite=True, ema_decay=0.9)
    acc = GradAccumulator(ps)
    loss = torch.ones((), device=dev())

    def group(bad_at=None):
        for j in range(2):
            for p in ps:
                p.grad = torch.randn(p.shape, generator=gen).to(dev())
            loss.fill_(float("nan") if j == bad_at else 1.0)
            acc.add(losses=[loss])
        # (the guard is handed no loss here: only the sticky word can tell it about micro-batch 1)
        opt.step(grads=acc, guard_words=[acc.sticky_word])
        acc.reset()

    group()                                                                        # moments and averages exist from here on
    before = state_bits(opt, ps, True)
    assert all(len(x) == 4 for x in before)
    group(bad_at=0)
    r = opt.grad_guard_record()
    assert same_state(before, state_bits(opt, ps, True))
    assert int(acc.sticky_word.item()) == 2
    assert r["skip"] == 4 and r["steps"] == 2 and r["skipped"] == 1 and r["skipped_consecutive"] == 1, r
    group()
    r = opt.grad_guard_record()
    assert int(acc.sticky_word.item()) == 0
    assert r["skip"] == 0 and r["steps"] == 3 and r["skipped"] == 1 and r["skipped_consecutive"] == 0, r
    assert not any(np.array_equal(x[0], y[0]) for x, y in zip(before, state_bits(opt, ps, True)))


def test_accumulator_refuses_a_changing_set_of_gradients(built):
    from multitask_hydranet_amd.optim import Adam, GradAccumulator
    ps = [torch.nn.Parameter(torch.ones(s, device=dev())) for s in [(5,), (1025,)]]
    acc = GradAccumulator(ps)
    opt = Adam(ps, 1e-2)
    with pytest.raises(RuntimeError):
        opt.step(grads=acc)                                                        # nothing pending
    for p in ps:
        p.grad = torch.ones_like(p)
    acc.add()
    ps[1].grad = None
    with pytest.raises(RuntimeError):
        acc.add()                                                                  # had a gradient in micro-batch 1, lacks one now
    assert acc.pending == 1
    acc.reset()
    acc.add()                                                                      # a new group may have another set
    ps[1].grad = torch.ones_like(ps[1])
    with pytest.raises(RuntimeError):
        acc.add()                                                                  # ... and the reverse
    acc.reset()
    acc.add()
    acc.add()
    assert acc.pending == 2 and np.array_equal(bits(acc.grad(ps[1])), bits(ps[1].grad))
