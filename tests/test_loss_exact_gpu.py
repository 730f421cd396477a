"""The loss kernels of csrc/hn_loss.hip and csrc/hn_det_loss.hip (and the pieces of csrc/hn_det_common.h they are built from) held to the
integer / float64 reference of tests/loss_ref.py through the C entry points, so that the test, not a wrapper, chooses the dispatch variant and k.
tests/test_loss_ref_cpu.py pins that reference to torch double and np.sort and checks the margins of the inputs used here.

Entry point and dispatch variant reached by each test
  test_seg_topk_select_exact / test_seg_topk_state_is_per_image
      hn_seg_loss_fwd: seg_ce_fwd_vec_kernel<5> (float target, HW % 4 == 0: HW 4, 200, 4100) or seg_ce_fwd_kernel (int64 target; HW 1,
      4098), seg_select_kernel levels 0..2 (lane-chunk edges, bin 0, the "fewer than k non-zero losses" branch), seg_hist_kernel levels
      1 and 2, seg_count_ties_kernel (two blocks per image at HW 4098 / 4100), seg_topk_sum_kernel, seg_loss_finalize_kernel;
      hn_seg_loss_bwd: seg_ce_bwd_kernel's tie share.
  test_seg_ce_values_and_gradients
      hn_seg_loss_fwd generic kernel at C 2, 3, 16, at ldl > C, at HW % 4 != 0, with an int64 target and with the logits 4 bytes off
      alignment at C = 5; the vector kernel at C = 5 otherwise; use_topk 0 and 1; hn_seg_loss_bwd at ldd = C and ldd > C.
  test_seg_gradient_in_space_to_depth_form
      hn_seg_loss_bwd_s2d: seg_ce_bwd_s2d_kernel (C = 3 / ldz 16, C = 5 with an int64 target, C = 5 at ldz 32) and
      seg_ce_bwd_s2d_vec_kernel<5, 24> (C = 5, float target, ldz 24).
  test_lane_ohem_select_exact / test_lane_dispatch_variants_agree
      hn_lane_cls_loss_fwd: lane_cls_fwd_reg_kernel<8> (M 384, 8192), <32> (M 8193, 32768), lane_cls_fwd_kernel (M 32769, and every M
      with the logits 4 bytes off alignment); hist_select_256 on injected bytes; hn_lane_cls_loss_bwd.
  test_focal_seg_loss             hn_seg_focal_fwd / _bwd, the powf branches (gamma 1.5, 1) and gamma 2, alpha 1 and 0.25, C 2, 5, 16.
  test_lane_loc_loss              hn_lane_loc_loss_fwd / _bwd at L 3, 33, 42, 322, M % 8 != 0.
  test_det_smooth_l1_loss         hn_det_loss_fwd / _bwd: det_loss_fwd_kernel<false, false, false>, det_loss_finalize_kernel<3, 4> with N
                                  on both sides of its 16-image pass, det_loss_bwd_kernel<false, false> with partial 256-anchor blocks.
  test_weighted_sum_*             hn_weighted_sum, forward and gradients, and its argument checks.

Injected bit patterns (loss_ref.seg_pattern / lane_pattern): a seg pixel with logits (0, -b, ..., -b), target 1 and cw[1] = 1 has the loss
b for any fp32 b >= 32, a lane row (-b, 0) the background log-prob -b.  Both are asserted on the arrays the kernels write (the loss array
in the workspace, lsm) before anything else, as a PRECONDITION; every selection assertion then takes the integer reference of the array
read back, so it demands the kernel's own threshold, remainder and tie count bit for bit.  On the MI355X the precondition holds for
every pattern as built: no pattern had to be rebuilt from other values.

The float64 focal reference clamps 1 - p at 0 (loss_ref.seg_focal): a saturated pixel has p = 1 + 1e-8 - O(e^-60) > 1 in float64, and a
fractional gamma has no real power of a negative base; for gamma 1 and 2 the clamp moves the loss by less than 1e-15.

Bounds and where they come from
  selection state (prefix, remaining, ties; lane aux[0..3], pmask)   exact
  seg scalar 1e-5 relative, dlogits 1e-4 of its maximum              test_seg_loss_topk_radix_select (fp32 F.cross_entropy alone is
                                                                     within 2e-8 / 3e-7 of float64 on these inputs, measured by
                                                                     test_loss_ref_cpu.py: nothing is widened)
  selection weight from dlogits 1e-6 relative                        three fp32 roundings (gout / denom, remaining / ties, their product)
  space-to-depth operand: <= 1 bf16 ulp, <= 1 % of elements differ   fp32 torch alone: <= 0.01 % (test_loss_ref_cpu.py)
  focal scalar 1e-5, dlogits 1e-4 of its maximum                     test_focal_seg_loss_kernels
  lane pos / neg / loc / gradients 2e-5 * max(|ref|, 1)              test_lane_losses_hip_vs_torch
  detection losses 2e-5 relative, dcls / dreg 2e-4 of the maximum    test_det_loss_matches_reference_loop
  weighted sum                                                       exact"""
import ctypes

import numpy as np
import pytest
import torch

from tests import loss_ref as R
from tests.guards import Guarded, dev

pytestmark = pytest.mark.gpu

GOUT = 3.0
SEG_SHAPES = ((3, 50, 82), (2, 33, 61), (2, 8, 12), (3, 66, 64))


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


def f32(x):
    return float(np.float32(x))


def to_dev(a, offset=0, fill=7.0):
    """numpy array -> contiguous device tensor whose address is `offset` elements past an aligned allocation"""
    t = torch.from_numpy(np.ascontiguousarray(a))
    buf = torch.full((offset + t.numel(),), fill, dtype=t.dtype, device=dev())
    v = buf[offset:].view(t.shape)
    v.copy_(t)
    return v


def padded_rows(a2d, ld, offset=0):
    """[M, C] numpy -> device view [M, C] with row stride ld, unrelated values in the ld - C columns between the rows"""
    M, C = a2d.shape
    buf = torch.full((offset + M * ld,), 7.0, device=dev())
    v = buf[offset:].view(M, ld)[:, :C]
    v.copy_(torch.from_numpy(np.ascontiguousarray(a2d)))
    return v


def close(got, want, rtol, name, floor=0.0):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    err = float(np.abs(got - want).max()) if got.size else 0.0
    bound = rtol * max(float(np.abs(want).max()) if want.size else 0.0, floor)
    print(f"{name}: max err {err:.3e} (bound {bound:.3e})")
    assert err <= bound, f"{name}: max error {err:.3e} > {bound:.3e}"


# ------------------------------------------------------------------------------------------------------------------------------------
# seg loss through the C entry points
# ------------------------------------------------------------------------------------------------------------------------------------
class SegRun:
    """hn_seg_loss_fwd on logits [N, HW, C] / target [N, HW], with everything it leaves in the workspace read back:
    loss fp32 [N, HW] | hist u32 [N * 2048] | state {prefix, remaining} [N] | ties u32 [N] | psum.  The workspace starts out as
    garbage: the call has to initialise what it reads."""

    def __init__(self, lib, logits, target, cw, tf, use_topk, k, ldl=None, offset=0):
        self.lib = lib
        self.N, self.HW, self.C = logits.shape
        self.M = self.N * self.HW
        self.ldl = ldl or self.C
        self.lg = padded_rows(logits.reshape(self.M, self.C), self.ldl, offset)
        tg = torch.from_numpy(np.ascontiguousarray(target.reshape(self.M))).to(dev())
        self.tg = tg.float().contiguous() if tf else tg.long().contiguous()
        self.cw = to_dev(np.asarray(cw, np.float32))
        self.tf, self.use_topk, self.k = int(tf), int(use_topk), int(k)
        self.ws = torch.full((lib.query("hn_seg_loss_ws_bytes", self.N, self.HW),), 0xA5, dtype=torch.uint8, device=dev())
        out = torch.full((1,), float("nan"), device=dev())
        lib.call("hn_seg_loss_fwd", self.lg.data_ptr(), self.ldl, self.C, self.tg.data_ptr(), self.tf, self.cw.data_ptr(), 255, self.N, self.HW,
                 self.use_topk, self.k, self.ws.data_ptr(), out.data_ptr())
        self.out = float(out.cpu()[0])
        raw = self.ws.cpu().numpy()
        o = self.M * 4 + self.N * 2048 * 4
        self.loss = raw[:self.M * 4].view(np.float32).reshape(self.N, self.HW).copy()
        self.state = raw[o:o + self.N * 8].view(np.uint32).reshape(self.N, 2).copy()
        self.ties = raw[o + self.N * 8:o + self.N * 12].view(np.uint32).copy()

    def head(self):
        return (self.lg.data_ptr(), self.ldl, self.C, self.tg.data_ptr(), self.tf, self.cw.data_ptr(), 255, self.N)

    def backward(self, gout=GOUT, ldd=None):
        ldd = ldd or self.C
        g = to_dev(np.array([gout], np.float32))
        dl = Guarded(self.M, self.C, ld=ldd)
        self.lib.call("hn_seg_loss_bwd", *self.head(), self.HW, self.use_topk, self.k, self.ws.data_ptr(), g.data_ptr(), dl.ptr(), ldd)
        d = dl.view.cpu().numpy().reshape(self.N, self.HW, self.C)
        dl.check("dlogits")
        return d

    def backward_s2d(self, H, W, ldz, gout=GOUT):
        g = to_dev(np.array([gout], np.float32))
        dz = Guarded(self.M // 4, ldz, dtype=torch.bfloat16)
        self.lib.call("hn_seg_loss_bwd_s2d", *self.head(), H, W, self.use_topk, self.k, self.ws.data_ptr(), g.data_ptr(), dz.ptr(), ldz)
        z = dz.view.float().cpu().numpy().reshape(self.N, H // 2, W // 2, ldz)
        dz.check("dz")
        return z

    def selection(self):
        """[(thr bits, remaining, ties)] per image, from the integer reference of the loss array the kernel wrote"""
        return [tuple(int(v) for v in R.topk_select(bits(self.loss[n]), self.k)) for n in range(self.N)]


def check_select(lib, images, k, tf, what):
    """one injected case: precondition, state bit for bit, the scalar, and the selection weight of every pixel from dlogits"""
    logits, target, cw = R.seg_inject(images)
    r = SegRun(lib, logits, target, cw, tf, 1, k)
    N, HW = target.shape
    inj = np.stack([np.where(ign, 0, b) for b, ign in images]).astype(np.float32)
    ign = np.stack([i for _, i in images])
    bad = bits(r.loss) != bits(inj)
    assert not bad.any(), (f"PRECONDITION, not the selection: {what}: {int(bad.sum())} injected losses were not reproduced, first "
                           f"{inj[bad][:3]} -> {r.loss[bad][:3]}")
    want = r.selection()
    got = [(int(r.state[n, 0]), int(r.state[n, 1]), int(r.ties[n])) for n in range(N)]
    assert got == want, f"{what}: (prefix, remaining, ties) per image {got} != {want}"
    total = 0.0
    for n, (thr, remaining, _) in enumerate(want):
        above = bits(r.loss[n]) > thr
        total += r.loss[n][above].astype(np.float64).sum() + remaining * float(np.array([thr], np.uint32).view(np.float32)[0])
    ref = total / (N * k)
    assert abs(r.out - ref) <= 1e-5 * abs(ref), f"{what}: out {r.out!r} != {ref!r}"
    d = r.backward()
    gs = f32(GOUT) * f32(1.0 / (N * k))
    wgt = d[:, :, 0].astype(np.float64) / gs
    wref = R.topk_weights(bits(r.loss), k)
    pix = (inj > 0) & ~ign
    err = np.abs(wgt - wref)[pix]
    assert (err <= 1e-6 * wref[pix]).all(), f"{what}: selection weight off by {err.max():.3e} (weights {np.unique(wref[pix])})"
    assert (d[ign] == 0).all(), f"{what}: an ignored pixel has a gradient"
    assert (d[~pix][:, 0] == 0).all() and float(np.abs(d[~pix]).max(initial=0.0)) <= 1e-12, f"{what}: a pixel with loss 0 has a gradient"


@pytest.mark.parametrize("tf", [1, 0], ids=["float_target", "int64_target"])
@pytest.mark.parametrize("HW", [1, 4, 200, 4098, 4100])
def test_seg_topk_select_exact(lib, HW, tf):
    """issue patterns 1..6 (and a fully ignored image), one image each"""
    ran = 0
    for name in R.SEG_PATTERNS:
        pat = R.seg_pattern(name, HW)
        if pat is None:
            continue
        b, ign, ks = pat
        for k in ks:
            check_select(lib, [(b, ign)], k, tf, f"{name} HW={HW} k={k}")
            ran += 1
    assert ran >= 2


@pytest.mark.parametrize("tf", [1, 0], ids=["float_target", "int64_target"])
@pytest.mark.parametrize("HW", [1, 4, 200, 4098, 4100])
def test_seg_topk_state_is_per_image(lib, HW, tf):
    """N = 3: two different patterns around a fully ignored image (threshold 0, contributes 0), at ranks built for either pattern"""
    names = [n for n in R.SEG_PATTERNS if n != "ignored" and R.seg_pattern(n, HW) is not None]
    for i, first in enumerate(names):
        last = names[(i + 1) % len(names)]
        p0, p1, p2 = R.seg_pattern(first, HW), R.seg_pattern("ignored", HW), R.seg_pattern(last, HW)
        for k in sorted(set(p0[2][:2] + p2[2][-2:])):
            check_select(lib, [p0[:2], p1[:2], p2[:2]], k, tf, f"{first}|ignored|{last} HW={HW} k={k}")


@pytest.mark.parametrize("C", [2, 3, 5, 16])
@pytest.mark.parametrize("n,h,w", SEG_SHAPES)
def test_seg_ce_values_and_gradients(lib, n, h, w, C):
    logits, target, cw = R.seg_case(0, C, n, h, w)
    loss64, _ = R.seg_ce(logits, target, cw)
    k, gap = R.choose_k(loss64)
    assert gap >= 5e-4
    refs = {t: R.seg_ce_mean(logits, target, cw, t, k) for t in (0, 1)}
    sel64 = [R.topk_select(loss64[i], k)[1:] for i in range(n)]
    for tf in (1, 0):
        for ldl, ldd in ((C, C), (C + 3, C + 3), (C, C + 3)):
            offsets = (0, 1) if (C == 5 and tf == 1 and ldl == C and (h * w) % 4 == 0) else (0,)       # 1: off alignment -> generic kernel
            for offset in offsets:
                for topk in (1, 0):
                    what = f"C={C} {(n, h, w)} tf={tf} ldl={ldl} ldd={ldd} offset={offset} topk={topk} k={k}"
                    r = SegRun(lib, logits, target, cw, tf, topk, k, ldl=ldl, offset=offset)
                    val, grad = refs[topk]
                    print(f"{what}: out {r.out!r} ref {val!r} rel {abs(r.out - val) / val:.2e}")
                    assert abs(r.out - val) <= 1e-5 * abs(val), what
                    close(r.loss, loss64, 1e-5, what + " per-pixel loss")
                    if topk:
                        got = [(int(r.state[i, 0]), int(r.state[i, 1]), int(r.ties[i])) for i in range(n)]
                        assert got == r.selection(), what
                        assert [g[1:] for g in got] == sel64, what             # the margin holds: fp32 selects what float64 selects
                    close(r.backward(ldd=ldd), grad * GOUT, 1e-4, what + " dlogits")


@pytest.mark.parametrize("C,tf,ldz,n,h,w", [(3, 1, 16, 3, 50, 82), (3, 0, 16, 2, 8, 12), (5, 0, 24, 3, 50, 82), (5, 0, 24, 2, 8, 12),
                                            (5, 1, 24, 3, 50, 82), (5, 1, 24, 2, 8, 12), (5, 1, 24, 3, 66, 64), (5, 1, 32, 2, 8, 12)])
def test_seg_gradient_in_space_to_depth_form(lib, C, tf, ldz, n, h, w):
    """generic kernel: C = 3, an int64 target, or ldz != 24; vector kernel: C = 5, float target, ldz = 24"""
    logits, target, cw = R.seg_case(0, C, n, h, w)
    k, _ = R.choose_k(R.seg_ce(logits, target, cw)[0])
    for topk in (1, 0):
        r = SegRun(lib, logits, target, cw, tf, topk, k)
        z = r.backward_s2d(h, w, ldz)
        _, grad = R.seg_ce_mean(logits, target, cw, topk, k)
        want = R.s2d_channels((grad * GOUT).reshape(-1, C), n, h, w, C, ldz)
        assert (z[..., 4 * C:] == 0).all(), "padding channels must be exactly zero"
        a, b = R.bf16_line(z), R.bf16_line(want)
        frac = float((a != b).mean())
        print(f"C={C} tf={tf} ldz={ldz} {(n, h, w)} topk={topk}: {100 * frac:.4f} % differ, max distance {int(np.abs(a - b).max())} bf16 ulp")
        assert int(np.abs(a - b).max()) <= 1 and frac <= 0.01


# ------------------------------------------------------------------------------------------------------------------------------------
# lane OHEM
# ------------------------------------------------------------------------------------------------------------------------------------
def lane_run(lib, z, t, ratio, offset=0, alpha=10.0, gpos=1.3, gneg=0.7):
    M = z.shape[0]
    zd, td = to_dev(z, offset), to_dev(t)
    lsm = torch.full((M, 2), float("nan"), device=dev())
    pmask = torch.full((M,), 0x5A, dtype=torch.uint8, device=dev())
    out, aux = torch.full((2,), float("nan"), device=dev()), torch.full((4,), float("nan"), device=dev())
    lib.call("hn_lane_cls_loss_fwd", zd.data_ptr(), td.data_ptr(), M, float(ratio), float(alpha), lsm.data_ptr(), pmask.data_ptr(), out.data_ptr(),
             aux.data_ptr())
    gp, gn = to_dev(np.array([gpos], np.float32)), to_dev(np.array([gneg], np.float32))
    dz = Guarded(M, 2)
    lib.call("hn_lane_cls_loss_bwd", lsm.data_ptr(), pmask.data_ptr(), aux.data_ptr(), gp.data_ptr(), gn.data_ptr(), float(alpha), M, dz.ptr())
    res = dict(lsm=lsm.cpu().numpy(), pmask=pmask.cpu().numpy(), out=out.cpu().numpy(), aux=aux.cpu().numpy(), dlogits=dz.view.cpu().numpy())
    dz.check("lane dlogits")
    return res


def lane_check(got, z, t, ratio, inj, what):
    ref = R.lane_cls(z, t, ratio, 10.0, gpos=1.3, gneg=0.7)
    assert (bits(got["lsm"][inj, 0]) == bits(z[inj, 0])).all(), f"PRECONDITION, not the selection: {what}: log p_bg of an injected row is not -b"
    assert (got["pmask"] == ref["pmask"]).all(), what
    assert [float(v) for v in got["aux"][1:]] == [float(ref["posn"]), float(ref["npos"]), float(ref["nneg"])], (what, got["aux"])
    thr = R.lane_select(got["lsm"][:, 0], ref["pmask"], ref["k"])
    assert bits(got["aux"][0]) == bits(thr), f"{what}: threshold {got['aux'][0]!r} != {thr!r} (rank {ref['k']} of {ref['nneg']})"
    for i, nm in enumerate(("pos", "neg")):
        assert abs(float(got["out"][i]) - ref[nm]) <= 2e-5 * max(abs(ref[nm]), 1.0), (what, nm, float(got["out"][i]), ref[nm])
    close(got["dlogits"], ref["dlogits"], 2e-5, what + " dlogits", floor=1.0)
    return ref


@pytest.mark.parametrize("name", R.LANE_PATTERNS)
@pytest.mark.parametrize("M", [384, 8192, 8193, 32768, 32769])
def test_lane_ohem_select_exact(lib, M, name):
    """aligned: reg<8> (M <= 8192), reg<32> (M <= 32768), generic above; the logits 4 bytes off alignment: the generic kernel at every M.
    The two runs see the same rows and must agree exactly on aux and pmask."""
    for z, t, ratio, inj in R.lane_pattern(name, M):
        what = f"{name} M={M} npos={int((t[:, 1] > 0).sum())}"
        a = lane_run(lib, z, t, ratio)
        ref = lane_check(a, z, t, ratio, inj, what)
        b = lane_run(lib, z, t, ratio, offset=1)
        lane_check(b, z, t, ratio, inj, what + " off alignment")
        assert (bits(a["aux"]) == bits(b["aux"])).all() and (a["pmask"] == b["pmask"]).all(), what
        if name == "no_negative":
            assert np.isposinf(a["aux"][0]) and float(a["out"][1]) == 0.0
        if name == "no_positive":
            assert ref["k"] == 1 and float(a["aux"][1]) == 1.0 and float(a["aux"][2]) == 0.0


@pytest.mark.parametrize("name", ["lowbyte", "topbyte", "ties"])
def test_lane_dispatch_variants_agree(lib, name):
    """the same 8192 rows through reg<8>, and with one more easy negative (log p_bg far above the threshold: rank and threshold do not
    move) through reg<32> and the generic kernel: aux[0..2] and pmask must be equal bit for bit, #neg one larger"""
    for z, t, ratio, inj in R.lane_pattern(name, 8192):
        z1 = np.concatenate([z, np.array([[5.0, 0.0]], np.float32)])
        t1 = np.concatenate([t, np.array([[1.0, 0.0]], np.float32)])
        r8, g8 = lane_run(lib, z, t, ratio), lane_run(lib, z, t, ratio, offset=1)
        r32, g32 = lane_run(lib, z1, t1, ratio), lane_run(lib, z1, t1, ratio, offset=1)
        for other, extra in ((g8, 0), (r32, 1), (g32, 1)):
            assert (bits(other["aux"][:3]) == bits(r8["aux"][:3])).all(), (name, r8["aux"], other["aux"])
            assert float(other["aux"][3]) == float(r8["aux"][3]) + extra
            assert (other["pmask"][:8192] == r8["pmask"]).all()


# ------------------------------------------------------------------------------------------------------------------------------------
# the remaining loss kernels against float64
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [2, 5, 16])
@pytest.mark.parametrize("alpha", [1.0, 0.25])
@pytest.mark.parametrize("gamma", [2.0, 1.5, 1.0])
def test_focal_seg_loss(lib, gamma, alpha, C):
    N, HW = 2, 4098
    logits, target, cw = R.focal_case(C, m=N * HW)
    val, grad = R.seg_focal(logits, target, cw, gamma, alpha)
    for tf in (1, 0):
        lg = padded_rows(logits, C + 3)
        tg = to_dev(target.astype(np.float32) if tf else target)
        cwd = to_dev(cw)
        ws = torch.full((lib.query("hn_seg_loss_blocks", N, HW),), float("nan"), device=dev())
        out = torch.full((1,), float("nan"), device=dev())
        lib.call("hn_seg_focal_fwd", lg.data_ptr(), C + 3, C, tg.data_ptr(), tf, cwd.data_ptr(), gamma, alpha, N, HW, ws.data_ptr(), out.data_ptr())
        g = to_dev(np.array([GOUT], np.float32))
        dl = Guarded(N * HW, C, ld=C + 3)
        lib.call("hn_seg_focal_bwd", lg.data_ptr(), C + 3, C, tg.data_ptr(), tf, cwd.data_ptr(), gamma, alpha, N, HW, g.data_ptr(), dl.ptr(), C + 3)
        got = float(out.cpu()[0])
        print(f"gamma={gamma} alpha={alpha} C={C} tf={tf}: out {got!r} ref {val!r} rel {abs(got - val) / val:.2e}")
        assert abs(got - val) <= 1e-5 * abs(val)
        d = dl.view.cpu().numpy()
        dl.check("focal dlogits")
        assert np.isfinite(d).all()
        close(d, grad * GOUT, 1e-4, "focal dlogits")


@pytest.mark.parametrize("L,M", [(3, 203), (33, 37), (42, 203), (322, 37)])
def test_lane_loc_loss(lib, L, M):
    for wcol in sorted({1, L - 2}):
        p, t, pmask, posn = R.lane_loc_case(L, M=M, wcol=wcol)
        val, grad, nrm = R.lane_loc(p, t, pmask, posn, wcol, gout=1.7)
        pd, td, pm = to_dev(p), to_dev(t), to_dev(pmask.astype(np.uint8), fill=0)
        aux = to_dev(np.array([0.0, posn, pmask.sum(), (~pmask).sum()], np.float32))
        rowloss, rownorm = Guarded(1, M), Guarded(1, M)
        out = torch.full((1,), float("nan"), device=dev())
        lib.call("hn_lane_loc_loss_fwd", pd.data_ptr(), td.data_ptr(), pm.data_ptr(), aux.data_ptr(), M, L, wcol, 10.0, rowloss.ptr(), rownorm.ptr(),
                 out.data_ptr())
        g = to_dev(np.array([1.7], np.float32))
        dp = Guarded(M, L)
        lib.call("hn_lane_loc_loss_bwd", pd.data_ptr(), td.data_ptr(), pm.data_ptr(), rownorm.ptr(), aux.data_ptr(), g.data_ptr(), M, L, wcol, 10.0,
                 dp.ptr())
        got = float(out.cpu()[0])
        assert abs(got - val) <= 2e-5 * max(abs(val), 1.0), (L, M, wcol, got, val)
        assert (rownorm.view.cpu().numpy()[0] == nrm).all()
        close(dp.view.cpu().numpy(), grad, 2e-5, f"L={L} M={M} wcol={wcol} dpred", floor=1.0)
        for gd, nm in ((rowloss, "rowloss"), (rownorm, "rownorm"), (dp, "dpred")):
            gd.check(nm)


@pytest.mark.parametrize("Kc", [1, 9])
@pytest.mark.parametrize("A", [1, 255, 257, 600])
@pytest.mark.parametrize("N", [1, 16, 17, 33])
def test_det_smooth_l1_loss(lib, N, A, Kc):
    cls, reg, anc, ann = R.det_case(N, A, Kc)
    ref = R.det_smooth_l1(cls, reg, anc, ann, gcls=1.0, greg=50.0)
    Mx = ann.shape[1]
    c, r, a, b = to_dev(cls), to_dev(reg), to_dev(anc), to_dev(ann)
    blocks = lib.query("hn_det_loss_blocks", A)
    assign = torch.full((N, A), -7, dtype=torch.int16, device=dev())
    part = torch.full((N, blocks, 3), float("nan"), device=dev())
    npos = torch.full((N,), float("nan"), device=dev())
    out = torch.full((2,), float("nan"), device=dev())
    lib.call("hn_det_loss_fwd", c.data_ptr(), r.data_ptr(), a.data_ptr(), b.data_ptr(), N, A, Kc, Mx, assign.data_ptr(), part.data_ptr(),
             npos.data_ptr(), out.data_ptr())
    g = to_dev(np.array([1.0, 50.0], np.float32))
    dcls, dreg = Guarded(N * A, Kc), Guarded(N * A, 4)
    lib.call("hn_det_loss_bwd", c.data_ptr(), r.data_ptr(), a.data_ptr(), b.data_ptr(), N, A, Kc, Mx, assign.data_ptr(), npos.data_ptr(),
             g.data_ptr(), dcls.ptr(), dreg.ptr())
    assert (assign.cpu().numpy() == ref["assign"]).all()
    assert npos.cpu().numpy().tolist() == [float(v) for v in ref["npos"]]
    got = out.cpu().numpy()
    print(f"N={N} A={A} K={Kc}: cls {got[0]!r} / {ref['cls']!r}  reg {got[1]!r} / {ref['reg']!r}  npos {ref['npos']}")
    for v, w in ((got[0], ref["cls"]), (got[1], ref["reg"])):
        assert abs(float(v) - w) <= 2e-5 * max(abs(w), 1e-6), (float(v), w)
    close(dcls.view.cpu().numpy().reshape(N, A, Kc), ref["dcls"], 2e-4, "dcls")
    close(dreg.view.cpu().numpy().reshape(N, A, 4), ref["dreg"], 2e-4, "dreg")
    dcls.check("dcls")
    dreg.check("dreg")


def weighted_sum_call(lib, x, w, gw, grp, gout, n=None):
    n = len(x) if n is None else n
    xd = to_dev(np.asarray(x, np.float32))
    ptrs = (ctypes.c_void_p * len(x))(*[xd.data_ptr() + 4 * i for i in range(len(x))])
    wa, ga = (ctypes.c_float * len(w))(*[float(v) for v in w]), (ctypes.c_float * len(gw))(*[float(v) for v in gw])
    ia = (ctypes.c_int * len(grp))(*[int(v) for v in grp])
    g = to_dev(np.array([gout], np.float32))
    out, grads = torch.full((1,), float("nan"), device=dev()), Guarded(1, len(x))
    lib.call("hn_weighted_sum", ctypes.addressof(ptrs), ctypes.addressof(wa), ctypes.addressof(ga), ctypes.addressof(ia), n, g.data_ptr(),
             out.data_ptr(), grads.ptr())
    res = out.cpu().numpy()[0], grads.view.cpu().numpy()[0]
    grads.check("grads")
    return res


@pytest.mark.parametrize("n,groups", [(1, 1), (5, 1), (5, 2), (5, 3), (8, 1), (8, 2), (8, 3)])
def test_weighted_sum_is_sequential_fp32(lib, n, groups):
    x, w, gw, grp = R.weighted_sum_case(n, groups)
    tot, grads = R.weighted_sum(x, w, gw, grp, gout=1.7)
    got, ggot = weighted_sum_call(lib, x, w, gw, grp, 1.7)
    assert bits(got) == bits(tot), (got, tot)
    assert (bits(ggot) == bits(grads)).all(), (ggot, grads)


def test_weighted_sum_argument_checks(lib):
    from multitask_hydranet_amd._lib import HipKernelError
    x, w, gw, grp = R.weighted_sum_case(8, 2)
    with pytest.raises(HipKernelError):
        weighted_sum_call(lib, list(x) + [1.0], list(w) + [1.0], gw, list(grp) + [1], 1.0)          # n = 9
    with pytest.raises(HipKernelError):
        weighted_sum_call(lib, x, w, gw, grp[::-1].copy(), 1.0)                                     # descending group ids
    torch.cuda.synchronize()
