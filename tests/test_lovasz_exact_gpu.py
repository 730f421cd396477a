"""The Lovasz kernels of csrc/hn_lovasz.hip held to exact order and per-pixel references through the C entry points.  The forward leaves
its intermediate results in the workspace (layout: tests/lovasz_ref.ws_layout, restated from the source's comment and held to
hn_seg_lovasz_ws_bytes by tests/test_lovasz_ref_cpu.py): the sorted keys and payloads of every class (keysB / valsB), the class and valid
counts, the fg count of every sorted tile, the loss partials and g = dloss/dp in pixel order (aliasing keysA).  They are read back and
checked as integers, so the device sort needs no reference implementation of expf.

After the forward (check_forward)
  counts    counts[c] and counts[C] are the integer fg and valid counts; every case asserts the V and the present classes it was DESIGNED
            for (tests/lovasz_cases.py), so no case can pass by having nothing to sort
  order     lovasz_ref.check_sorted on every class: (key, pixel) strictly increasing, the first V payloads exactly the valid pixels,
            bit 31 = (label == c), float(key) within 4e-6 relative of float64 d, the tail 0x3FFFFFFF; palette and saturated inputs: the
            payload equals the float64 stable order EXACTLY (continuous logits: properties only)
  blkfg     the fg count of sorted tile b below V; 0 for an absent class
  weights   g[pixel][c] = -+weights(...) at the pixel's rank in the device's own payload, within 2^-20 relative (the fp32 form has at
            most five roundings and a division; a numpy fp32 restatement stays within 1 ulp up to 8.4 M pixels, 8 ulp leaves room for a
            division that is not correctly rounded), exactly +0.0 where the key is >= 1.0f
  loss      sum_c sum_j (1 - key_j) weight_j / n_present in float64 from the device's sorted keys within 2^-18 relative (about 47 fp32
            roundings of positive terms per tile partial; the finalize runs in double), and lovasz_softmax_ref within 1e-5
After the plain backward, gout = 3 (check_backward)
  every component |dl - pixel_grad| <= 4e-6 * |scale| p_c (|g_c| + sum_k p_k |g_k|), pixel_grad from the device's g and a float64
  softmax (a numpy fp32 restatement reaches 9.5e-7 at C = 16 on N(0, 2) logits; four times that leaves room for the device expf);
  ignored pixels, masked images and the no-class-present case are WRITTEN as +0.0 bit for bit; the padding columns keep their sentinel;
  the backward leaves the workspace as it found it
After the space-to-depth backward (check_s2d)
  every bf16 within half a bf16 step plus the fp32 bound of the plain backward's value (exact_checks.bf_interval); channels [4C, ldz)
  and dropped pixels +0.0 bit for bit
The workspace is a GuardedBytes of exactly hn_seg_lovasz_ws_bytes and every output a NaN-filled Guarded; every band is checked after
every call.

Measured on the MI355X (largest value over all cases; printed by every test)
  key against float64 d          7.5e-7 relative (check_sorted's bound: 4e-6)
  weight                         1.2e-7 relative (bound 2^-20 = 9.5e-7)
  loss against the sorted keys   7.8e-8 relative (bound 2^-18 = 3.8e-6)
  dlogits component              9.7e-7 of its magnitude |scale| p_c (|g_c| + sum_k p_k |g_k|) (bound 4e-6), at C = 16
The whole file takes 15 s, of which the two 8.4 M-pixel cases take 5.7 and 6.0 s (host-side float64 checks); every other case is under
half a second.

Shown to bite on one-line mutations of a copy of the kernel: `carry = tot` in lv_post_kernel fails the weights check of every case with
more than 512 valid pixels (first bad rank 512), `(float)(G - F - 1)` the weights check of every case but P = 1 and the two without a
present class.  A mutation that breaks the sort itself leaves sorted slots unwritten; lv_post_kernel scatters g by the payload, so such a
mutant must bound that store before it is run.  check_sorted's own bite is shown on the host (test_lovasz_ref_cpu.py).

Kernels and branches reached by each test
  test_wave_round_and_tile_edges        P = 1, 63, 64, 65, 255, 256, 257, 8191, 8192, 8193, 3 * 8192 + 5, all valid, lv_key_kernel<5> and
                                        the three radix passes with a last wave / round / tile that is full, one short and one over
  test_valid_count_on_a_tile_edge       V = 8192 and 8193 of 16384 interleaved pixels: lv_post_kernel's early exit, lv_fgcount's j < V
  test_saturated_logits                 only keys 0.0 and 1.0: every item in one digit bin per pass; g = 0 on the d >= 1 side
  test_continuous_logits                N(0, 2) logits: every radix pass spreads over its bins; properties only
  test_class_counts                     C = 2, 15, 16 (lv_*_kernel<0>; 16 takes the key kernel's LDS opt-in), C = 5, at two tiles, ldl > C
  test_row_strides                      ldl = C + 3, ldd = C + 1, ldz = 4C and 4C + 4
  test_label_forms                      float32 and int64 labels: 255, -1, C + 2, 254, 2.7
  test_present_sets                     an absent class, exactly one present class, none present, nothing valid
  test_masked_entry_points              hn_seg_lovasz_*_masked at N = 3, masks 111 / 101 / 001 / 000
  test_scan_second_trip                 1026 tiles: lv_scan_kernel's second trip and its carry
  test_backward_grid_stride_loops       8 405 000 pixels: both backward kernels' grid-stride loops repeat (grids capped at 8192)
  test_two_runs_are_bit_identical       the whole workspace, loss and gradients
  test_refused_calls                    every HN_CHECK_ARG of the three entry points, before any launch"""
import time

import numpy as np
import pytest
import torch

from tests import exact_checks as X, lovasz_cases as L, lovasz_ref as R
from tests.guards import SENT16, SENT32, Guarded, GuardedBytes, dev
from tests.loss_ref import s2d_channels
from tests.lovasz_ref import lovasz_softmax_ref

pytestmark = pytest.mark.gpu

GOUT = 3.0
W_TOL = 2.0 ** -20
LOSS_TOL = 2.0 ** -18
GRAD_TOL = 4e-6
UNDERFLOW = 1e-37              # below fp32's smallest normal number: no relative bound can hold there
WORST = dict(weight=0.0, loss=0.0, grad=0.0, key=0.0)


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    import __graft_entry__ as g
    g.build()
    from multitask_hydranet_amd._lib import lib
    yield lib()
    print("lovasz exact, largest values reached: " + ", ".join(f"{k} {v:.3e}" for k, v in WORST.items()))


def worst(kind, v):
    WORST[kind] = max(WORST[kind], float(v))


def padded(a2d, ld):
    """[M, C] numpy -> device view [M, C] with row stride ld, unrelated values in the ld - C columns between the rows"""
    M, C = a2d.shape
    buf = torch.full((M * ld,), 7.0, device=dev())
    v = buf.view(M, ld)[:, :C]
    v.copy_(torch.from_numpy(a2d))
    return v


class Run:
    """hn_seg_lovasz_fwd[_masked] on a Case, with everything it leaves in the workspace read back; backward() and backward_s2d() on the
    same workspace.  unmasked=True calls the entry points without a mask (the case's mask must be None or all ones)."""

    def __init__(self, lib, cs, unmasked=None):
        self.lib, self.cs = lib, cs
        n, hw, c, P = cs.n, cs.hw, cs.c, cs.P
        self.masked = cs.mask is not None if unmasked is None else not unmasked
        assert self.masked or cs.mask is None or all(cs.mask)
        self.lay = R.ws_layout(n, hw, c)
        assert self.lay["total"] == lib.query("hn_seg_lovasz_ws_bytes", n, hw, c)
        self.lg = padded(cs.logits.reshape(P, c), cs.ldl)
        self.tg = torch.from_numpy(cs.labels.reshape(P)).to(dev())
        self.tf = int(cs.labels.dtype == np.float32)
        self.vm = torch.tensor(list(cs.mask), dtype=torch.uint8, device=dev()) if self.masked else None
        self.sfx, self.va = ("_masked", (self.vm.data_ptr(),)) if self.masked else ("", ())
        self.head = (self.lg.data_ptr(), cs.ldl, c, self.tg.data_ptr(), self.tf, L.IGNORE, n)
        self.ws = GuardedBytes(self.lay["total"])
        out = Guarded(1, 1)
        lib.call("hn_seg_lovasz_fwd" + self.sfx, *self.head, hw, *self.va, self.ws.ptr(), out.ptr())
        torch.cuda.synchronize()
        self.ws.check(f"{cs.name}: workspace after the forward")
        out.check(f"{cs.name}: loss")
        self.out = out.view.cpu().numpy().reshape(1).copy()
        self.raw = self.ws.view.cpu().numpy().copy()
        nblk = self.lay["nblk"]
        self.keys = self.arr("keysB", np.uint32, c * P).reshape(c, P)
        self.vals = self.arr("valsB", np.uint32, c * P).reshape(c, P)
        self.g = self.arr("keysA", np.float32, P * c).reshape(P, c)
        self.counts = self.arr("counts", np.uint32, 32)
        self.blkfg = self.arr("blkfg", np.uint32, c * nblk).reshape(c, nblk)
        self.gout = torch.tensor([GOUT], device=dev())

    def arr(self, name, dtype, count):
        o = self.lay[name]
        return self.raw[o:o + 4 * count].view(dtype)

    def ws_unchanged(self, what):
        assert torch.equal(self.ws.view.cpu(), torch.from_numpy(self.raw)), f"{self.cs.name}: {what} wrote into the workspace"

    def backward(self):
        cs = self.cs
        dl = Guarded(cs.P, cs.c, cs.ldd)
        self.lib.call("hn_seg_lovasz_bwd" + self.sfx, *self.head, cs.hw, *self.va, self.ws.ptr(), self.gout.data_ptr(), dl.ptr(), cs.ldd)
        torch.cuda.synchronize()
        dl.check(f"{cs.name}: dlogits")
        self.ws.check(f"{cs.name}: workspace after the backward")
        self.ws_unchanged("the backward")
        return dl.view.cpu().numpy().copy()

    def backward_s2d(self):
        cs = self.cs
        dz = Guarded(cs.P // 4, cs.ldz, dtype=torch.bfloat16)
        self.lib.call("hn_seg_lovasz_bwd_s2d" + self.sfx, *self.head, cs.h, cs.w, *self.va, self.ws.ptr(), self.gout.data_ptr(), dz.ptr(), cs.ldz)
        torch.cuda.synchronize()
        dz.check(f"{cs.name}: dz")
        self.ws.check(f"{cs.name}: workspace after the space-to-depth backward")
        return dz.view.cpu().contiguous()


def check_forward(run, ref_loss=True):
    """-> (present bool [C], n_present); everything the forward leaves, against the integer / float64 restatement"""
    cs = run.cs
    c, P, nblk = cs.c, cs.P, run.lay["nblk"]
    lab, valid = cs.effective()
    assert cs.observed() == (cs.V, cs.present), (cs.name, cs.observed())
    V = cs.V
    G = np.array([int((valid & (lab == k)).sum()) for k in range(c)])
    want_counts = np.zeros(32, np.int64)
    want_counts[:c], want_counts[c] = G, V
    assert run.counts.astype(np.int64).tolist() == want_counts.tolist(), (cs.name, run.counts[:c + 1].tolist(), G.tolist(), V)
    present = G > 0
    assert tuple(np.flatnonzero(present)) == cs.present
    x = cs.logits.reshape(P, c)
    tile = np.arange(V) // R.TILE
    total, g_seen = 0.0, np.zeros((P, c), bool)
    for k in range(c):
        keys, vals = run.keys[k], run.vals[k]
        d64 = R.key_d(x, lab, k)
        R.check_sorted(keys, vals, lab, valid, k, d64)
        pix = (vals[:V] & 0x7FFFFFFF).astype(np.int64)
        kf = keys[:V].view(np.float32).astype(np.float64)
        want = d64[pix]
        if V:
            worst("key", (np.abs(kf - want) / np.maximum(want, 1e-30))[np.abs(kf - want) > 1e-37].max(initial=0.0))
        if cs.kind != "continuous":
            order = cs.order(k, d64)
            bad = np.flatnonzero(vals != order)
            assert bad.size == 0, (f"{cs.name}: class {k}: {bad.size} payloads differ from the float64 stable order, first at sorted position "
                                   f"{bad[0]}: got 0x{int(vals[bad[0]]):08x} want 0x{int(order[bad[0]]):08x}")
        fg = (vals[:V] >> 31).astype(bool)
        want_blk = np.bincount(tile[fg], minlength=nblk) if present[k] else np.zeros(nblk, np.int64)
        assert run.blkfg[k].astype(np.int64).tolist() == want_blk.tolist(), (cs.name, k, run.blkfg[k].tolist(), want_blk.tolist())
        if not present[k]:
            continue
        F, B, w = R.weights(fg, int(G[k]))
        zero = keys[:V] >= R.ONE_KEY
        want_g = np.where(zero, 0.0, np.where(fg, -w, w))
        got_g = run.g[pix, k]
        g_seen[pix, k] = True
        err = np.abs(got_g.astype(np.float64) - want_g)
        worst("weight", (err / np.maximum(np.abs(want_g), 1e-300)).max())
        bad = np.flatnonzero(~(err <= W_TOL * np.abs(want_g)))
        assert bad.size == 0, (f"{cs.name}: class {k}: {bad.size} weights outside 2^-20, first at rank {bad[0]} (pixel {pix[bad[0]]}, F {F[bad[0]]}, "
                               f"B {B[bad[0]]}, G {G[k]}): got {got_g[bad[0]]!r} want {want_g[bad[0]]!r}")
        assert (got_g[zero].view(np.uint32) == 0).all(), f"{cs.name}: class {k}: g is not +0.0 where the key is >= 1.0f"
        total += float(((1.0 - kf) * w).sum())
    assert (g_seen == (valid[:, None] & present[None, :])).all()
    npres = int(present.sum())
    got = float(run.out[0])
    if npres == 0:
        assert run.out.view(np.uint32)[0] == 0, (cs.name, got)
    else:
        want = total / npres
        rel = abs(got - want) / want
        worst("loss", rel)
        print(f"{cs.name}: loss {got!r}, from the sorted keys {want!r} (rel {rel:.2e})")
        assert rel <= LOSS_TOL, (cs.name, got, want, rel)
    if ref_loss:
        t = torch.from_numpy(np.where(valid, lab, L.IGNORE).reshape(cs.n, cs.h, cs.w))
        ref = float(lovasz_softmax_ref(torch.from_numpy(cs.logits).permute(0, 3, 1, 2), t))
        assert abs(got - ref) <= 1e-5 * abs(ref), (cs.name, got, ref)
    return present, npres


def grad_reference(run, present, npres):
    """-> (float64 pixel_grad from the device's g, its 4e-6 bound), zeros at dropped pixels.  The bound carries the absolute 1e-37 that
    check_sorted gives the keys: a saturated pixel's p_c is 1e-87 in float64 and 0 in any fp32 evaluation"""
    cs = run.cs
    _, valid = cs.effective()
    if npres == 0:
        z = np.zeros((cs.P, cs.c))
        return z, z
    x = cs.logits.reshape(cs.P, cs.c)
    scale = GOUT / npres
    g = np.where(valid[:, None] & present[None, :], run.g.astype(np.float64), 0.0)        # (elsewhere g holds stale keys, never read)
    want = np.where(valid[:, None], R.pixel_grad(x, g, present, scale), 0.0)
    bound = np.where(valid[:, None], GRAD_TOL * R.pixel_grad_mag(x, g, present, scale) + UNDERFLOW, 0.0)
    return want, bound


def check_backward(run, present, npres):
    """-> (the device's dlogits fp32 [P, C], the bound)"""
    cs = run.cs
    _, valid = cs.effective()
    dl = run.backward()
    want, bound = grad_reference(run, present, npres)
    err = np.abs(dl.astype(np.float64) - want)
    if npres:
        worst("grad", (err[valid] / np.maximum((bound[valid] - UNDERFLOW) / GRAD_TOL, 1e-30)).max(initial=0.0))
    bad = np.argwhere(~(err <= bound))
    assert bad.size == 0, (f"{cs.name}: {len(bad)} dlogits components outside their bound, first at pixel {bad[0][0]} class {bad[0][1]}: got "
                           f"{dl[tuple(bad[0])]!r} want {want[tuple(bad[0])]!r} (bound {bound[tuple(bad[0])]:.3e})")
    dropped = ~valid if npres else np.ones(cs.P, bool)
    assert (dl[dropped].view(np.uint32) == 0).all(), f"{cs.name}: a dropped pixel's dlogits are not +0.0 bit for bit"
    if npres and cs.kind != "saturated":                 # (saturated: p is exactly 0 or 1 and the softmax Jacobian vanishes)
        assert np.abs(dl[valid]).max() > 0
    return dl, bound


def check_s2d(run, dl, bound):
    cs = run.cs
    _, valid = cs.effective()
    dz = run.backward_s2d()                                                              # bf16 [P / 4, ldz]
    y = s2d_channels(dl.astype(np.float64), cs.n, cs.h, cs.w, cs.c, cs.ldz).reshape(-1, cs.ldz)
    s = s2d_channels(bound, cs.n, cs.h, cs.w, cs.c, cs.ldz).reshape(-1, cs.ldz)
    X.bf_interval(dz, torch.from_numpy(y), torch.from_numpy(s), f"{cs.name}: dz")
    live = s2d_channels(np.broadcast_to((valid & bool(len(cs.present)))[:, None], (cs.P, cs.c)).astype(np.float64), cs.n, cs.h, cs.w, cs.c,
                        cs.ldz).reshape(-1, cs.ldz) > 0
    zbits = dz.view(torch.int16).numpy()
    assert (zbits[~live] == 0).all(), f"{cs.name}: channels [4C, ldz) or dropped pixels of dz are not +0.0 bit for bit"
    return dz


def full_check(lib, cs, ref_loss=True, unmasked=None):
    t0 = time.time()
    run = Run(lib, cs, unmasked)
    present, npres = check_forward(run, ref_loss)
    dl, bound = check_backward(run, present, npres)
    dz = check_s2d(run, dl, bound) if cs.s2d else None
    print(f"{cs.name}: P {cs.P} V {cs.V} present {cs.present} s2d {cs.s2d}: {time.time() - t0:.2f} s; worst so far {WORST}")
    return run, dl, dz


@pytest.mark.parametrize("P", L.EDGE_P)
def test_wave_round_and_tile_edges(lib, P):
    full_check(lib, L.edge_case(P))
    if P in (8191, 8192, 8193):
        full_check(lib, L.edge_case(P, tf=P % 2 == 0))                                   # (the other label type)


@pytest.mark.parametrize("extra", [0, 1])
def test_valid_count_on_a_tile_edge(lib, extra):
    run, _, _ = full_check(lib, L.tile_edge_valid(extra))
    part = run.arr("part", np.float32, 5 * 2).reshape(5, 2)
    if not extra:
        assert (part[:, 1].view(np.uint32) == 0).all() and (run.blkfg[:, 1] == 0).all()  # the fully ignored tile: partial written as 0
    assert (part[:, 0] > 0).all()


def test_saturated_logits(lib):
    run, dl, _ = full_check(lib, L.saturated_case())
    assert set(np.unique(run.keys).tolist()) == {0, R.ONE_KEY}
    for k in range(5):
        zero = run.keys[k] == R.ONE_KEY
        assert 8192 < zero.sum() < run.cs.P - 8192
        assert not run.g[run.vals[k][zero] & 0x7FFFFFFF, k].view(np.uint32).any() and run.g[run.vals[k][~zero] & 0x7FFFFFFF, k].all()


@pytest.mark.parametrize("P,tf", [(8193, True), (3 * 8192 + 5, False)])
def test_continuous_logits(lib, P, tf):
    run, _, _ = full_check(lib, L.continuous_case(P, 5, tf))
    digits = [len(np.unique((run.keys >> s) & 1023)) for s in (0, 10, 20)]               # every radix pass spreads over many bins
    assert digits[0] == 1024 and digits[1] == 1024 and digits[2] >= 64, digits


@pytest.mark.parametrize("kind", ["palette", "continuous"])
@pytest.mark.parametrize("c", [2, 5, 15, 16])
def test_class_counts(lib, c, kind):
    full_check(lib, L.class_count_case(c, kind))


@pytest.mark.parametrize("ldz_extra", [0, 4])
def test_row_strides(lib, ldz_extra):
    cs = L.stride_case(ldz_extra)
    assert (cs.ldl, cs.ldd, cs.ldz) == (8, 6, 20 + ldz_extra) and cs.s2d
    run, dl, dz = full_check(lib, cs)
    dense = L.stride_case(ldz_extra)
    dense.ldl, dense.ldd = dense.c, dense.c
    run2 = Run(lib, dense)
    assert np.array_equal(run.raw, run2.raw) and np.array_equal(run.out.view(np.uint32), run2.out.view(np.uint32))
    assert np.array_equal(dl.view(np.uint32), run2.backward().view(np.uint32))


@pytest.mark.parametrize("tf", [True, False])
def test_label_forms(lib, tf):
    run, dl, dz = full_check(lib, L.label_forms_case(tf))
    other = Run(lib, L.label_forms_case(not tf))                                         # 2.7 is class 2, 254.0 is 254: the same bits
    assert np.array_equal(run.raw, other.raw) and np.array_equal(run.out.view(np.uint32), other.out.view(np.uint32))


@pytest.mark.parametrize("which", ["absent", "one", "none", "ignored"])
def test_present_sets(lib, which):
    run, dl, dz = full_check(lib, L.present_case(which))
    if which in ("none", "ignored"):
        assert run.out.view(np.uint32)[0] == 0 and not dl.view(np.uint32).any() and not dz.view(torch.int16).numpy().any()


@pytest.mark.parametrize("tf", [True, False])
def test_masked_entry_points(lib, tf):
    base, masked = L.masked_cases(tf)
    plain = full_check(lib, base)
    for cs in masked:
        run, dl, dz = full_check(lib, cs)
        _, valid = cs.effective()
        assert cs.V == 0 or not dl[~valid].view(np.uint32).any()
        if all(cs.mask):                                                                 # 111: the unmasked call bit for bit
            assert np.array_equal(run.raw, plain[0].raw), "the workspace (sorted payload included) differs from the unmasked call's"
            assert np.array_equal(run.out.view(np.uint32), plain[0].out.view(np.uint32))
            assert np.array_equal(dl.view(np.uint32), plain[1].view(np.uint32)) and torch.equal(dz.view(torch.int16), plain[2].view(torch.int16))


def test_scan_second_trip(lib):
    cs = L.big_case(4098, "continuous", True)
    assert R.ws_layout(cs.n, cs.hw, cs.c)["nblk"] == 1026 > 1024 and cs.P // 4 == 2100225
    full_check(lib, cs)


def test_backward_grid_stride_loops(lib):
    cs = L.big_case(4100, "palette", False)
    assert cs.P == 8405000 > 8192 * 256 * 4 and R.ws_layout(cs.n, cs.hw, cs.c)["nblk"] == 1027
    full_check(lib, cs)


def test_two_runs_are_bit_identical(lib):
    for cs in (L.tile_edge_valid(1), L.continuous_case(3 * 8192 + 5, 5, False), L.masked_cases(True)[1][1]):
        a, b = Run(lib, cs), Run(lib, cs)
        assert np.array_equal(a.raw, b.raw), cs.name
        assert np.array_equal(a.out.view(np.uint32), b.out.view(np.uint32))
        assert np.array_equal(a.backward().view(np.uint32), b.backward().view(np.uint32))
        if cs.s2d:
            assert torch.equal(a.backward_s2d().view(torch.int16), b.backward_s2d().view(torch.int16))


def test_refused_calls(lib):
    """every refusal is an HN_CHECK_ARG in front of the first launch (seg_lovasz_fwd, seg_lovasz_bwd, seg_lovasz_bwd_s2d and the masked
    wrappers): error code 1, and the loss, gradients and workspace keep their sentinels"""
    n, h, w, c = 2, 4, 6, 5
    hw, P = h * w, n * h * w
    lg = torch.zeros((P, 17), device=dev())
    tg = torch.zeros((P,), dtype=torch.int64, device=dev())
    vm = torch.ones((n,), dtype=torch.uint8, device=dev())
    gout = torch.tensor([GOUT], device=dev())
    ws = GuardedBytes(lib.query("hn_seg_lovasz_ws_bytes", n, hw, 16))
    out, dl, dz = Guarded(1, 1), Guarded(P, 17), Guarded(P // 4, 68, dtype=torch.bfloat16)
    r = lib.raw
    LG, TG, VM, GO, WS, O, DL, DZ = lg.data_ptr(), tg.data_ptr(), vm.data_ptr(), gout.data_ptr(), ws.ptr(), out.ptr(), dl.ptr(), dz.ptr()
    big_n, big_hw = 2, 1 << 30                                                          # N * HW = 2^31: the payload has 31 index bits
    refused = {
        "fwd C=1": r("hn_seg_lovasz_fwd")(LG, 5, 1, TG, 0, 255, n, hw, WS, O, None),
        "fwd C=17": r("hn_seg_lovasz_fwd")(LG, 17, 17, TG, 0, 255, n, hw, WS, O, None),
        "fwd ldl<C": r("hn_seg_lovasz_fwd")(LG, c - 1, c, TG, 0, 255, n, hw, WS, O, None),
        "fwd 2^31": r("hn_seg_lovasz_fwd")(LG, c, c, TG, 0, 255, big_n, big_hw, WS, O, None),
        "fwd N=0": r("hn_seg_lovasz_fwd")(LG, c, c, TG, 0, 255, 0, hw, WS, O, None),
        "fwd_masked null valid": r("hn_seg_lovasz_fwd_masked")(LG, c, c, TG, 0, 255, n, hw, None, WS, O, None),
        "fwd_masked C=17": r("hn_seg_lovasz_fwd_masked")(LG, 17, 17, TG, 0, 255, n, hw, VM, WS, O, None),
        "bwd C=1": r("hn_seg_lovasz_bwd")(LG, 5, 1, TG, 0, 255, n, hw, WS, GO, DL, 5, None),
        "bwd C=17": r("hn_seg_lovasz_bwd")(LG, 17, 17, TG, 0, 255, n, hw, WS, GO, DL, 17, None),
        "bwd ldl<C": r("hn_seg_lovasz_bwd")(LG, c - 1, c, TG, 0, 255, n, hw, WS, GO, DL, c, None),
        "bwd ldd<C": r("hn_seg_lovasz_bwd")(LG, c, c, TG, 0, 255, n, hw, WS, GO, DL, c - 1, None),
        "bwd 2^31": r("hn_seg_lovasz_bwd")(LG, c, c, TG, 0, 255, big_n, big_hw, WS, GO, DL, c, None),
        "bwd_masked null valid": r("hn_seg_lovasz_bwd_masked")(LG, c, c, TG, 0, 255, n, hw, None, WS, GO, DL, c, None),
        "s2d C=1": r("hn_seg_lovasz_bwd_s2d")(LG, 5, 1, TG, 0, 255, n, h, w, WS, GO, DZ, 20, None),
        "s2d C=17": r("hn_seg_lovasz_bwd_s2d")(LG, 17, 17, TG, 0, 255, n, h, w, WS, GO, DZ, 68, None),
        "s2d ldl<C": r("hn_seg_lovasz_bwd_s2d")(LG, c - 1, c, TG, 0, 255, n, h, w, WS, GO, DZ, 20, None),
        "s2d odd H": r("hn_seg_lovasz_bwd_s2d")(LG, c, c, TG, 0, 255, n, h + 1, w, WS, GO, DZ, 20, None),
        "s2d odd W": r("hn_seg_lovasz_bwd_s2d")(LG, c, c, TG, 0, 255, n, h, w - 1, WS, GO, DZ, 20, None),
        "s2d ldz<4C": r("hn_seg_lovasz_bwd_s2d")(LG, c, c, TG, 0, 255, n, h, w, WS, GO, DZ, 4 * c - 1, None),
        "s2d 2^31": r("hn_seg_lovasz_bwd_s2d")(LG, c, c, TG, 0, 255, 2, 1 << 15, 1 << 15, WS, GO, DZ, 20, None),
        "s2d_masked null valid": r("hn_seg_lovasz_bwd_s2d_masked")(LG, c, c, TG, 0, 255, n, h, w, None, WS, GO, DZ, 20, None),
    }
    torch.cuda.synchronize()
    assert all(v == 1 for v in refused.values()), {k: v for k, v in refused.items() if v != 1}
    assert ws.untouched(), "a refused call wrote into the workspace"
    ws.check("refused calls: workspace")
    for o, name, sent in ((out, "loss", SENT32), (dl, "dlogits", SENT32), (dz, "dz", SENT16)):
        o.check("refused calls: " + name)
        bits = o.view.contiguous().view(torch.int32 if sent == SENT32 else torch.int16)
        assert bool((bits == sent).all()), f"a refused call wrote {name}"
