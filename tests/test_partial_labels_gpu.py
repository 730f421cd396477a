"""GPU: the losses under per-image task masks (gt_dict["task_valid"]) against tests/partial_ref.py -- the existing float64 /
integer references applied to the sub-batch of labelled images, gradients scattered back into zeros.

The C entry points (`hn_*_masked`) are called where the dispatch variant matters, with NaN-prefilled outputs (tests/guards.py): an
unlabelled image's gradient has to be WRITTEN as 0.0.  Masks at N = 3: 111, 101, 001, 000; at N = 17 one with ones on both sides of the
detection finalize's 16-image pass.  Bounds are the unmasked tests' own (test_loss_exact_gpu.py, test_det_iou_gpu.py, test_lovasz_gpu.py):
seg scalar 1e-5 relative, dlogits 1e-4 of its maximum, selection state exact per labelled image; detection losses and pos_iou 2e-5
relative, dcls / dreg 2e-4 of the maximum, npos and assign exact; lane aux and pmask exact against the integer reference of the labelled
rows of the lsm read back, pos / neg / loc / gradients 2e-5 max(|ref|, 1).  For every task: the all-ones mask equals the unmasked entry
point bit for bit, two runs are bit-identical, one captured graph replayed with other mask contents gives those masks' eager bits."""
import copy

import numpy as np
import pytest
import torch

from tests import det_atss_ref, loss_ref as R, partial_ref as P
from tests.guards import Guarded, dev
from tests.helpers import load_cfg, load_npz, tiny_state
from tests.test_loss_exact_gpu import SEG_SHAPES, bits, close, padded_rows, to_dev

pytestmark = pytest.mark.gpu

GOUT = 3.0
MASKS3 = ((1, 1, 1), (1, 0, 1), (0, 0, 1), (0, 0, 0))
MASK17 = (1, 0, 1, 1, 0, 0, 1, 0, 1, 1, 0, 1, 0, 0, 1, 0, 1)             # images 0..15 are the finalize's first pass, image 16 its second


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    import __graft_entry__ as g
    g.build()
    from multitask_hydranet_amd._lib import lib
    return lib()


@pytest.fixture(scope="module")
def K(lib):
    from multitask_hydranet_amd import ops
    return ops


def masks_for(n):
    if n == 17:
        return (MASK17, (1,) * 17)
    return tuple(dict.fromkeys(m[:n] for m in MASKS3))


def vmask(m):
    return torch.tensor(list(m), dtype=torch.uint8, device=dev())


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


# ------------------------------------------------------------------------------------------------------------------------------------
# seg CE / top-k
# ------------------------------------------------------------------------------------------------------------------------------------
def seg_run(lib, logits, target, cw, tf, topk, k, mask, offset=0, s2d=None, ldz=24):
    """hn_seg_loss_fwd(_masked) + bwd(_masked) [+ bwd_s2d(_masked)]; mask None = the unmasked entry points"""
    N, HW, C = logits.shape
    M = N * HW
    lg = padded_rows(logits.reshape(M, C), C, offset)
    tg = torch.from_numpy(np.ascontiguousarray(target.reshape(M))).to(dev())
    tg = tg.float().contiguous() if tf else tg.long().contiguous()
    cwd = to_dev(np.asarray(cw, np.float32))
    ws = torch.full((lib.query("hn_seg_loss_ws_bytes", N, HW),), 0xA5, dtype=torch.uint8, device=dev())
    out = torch.full((1,), float("nan"), device=dev())
    v = None if mask is None else vmask(mask)
    sfx, va = ("", ()) if mask is None else ("_masked", (v.data_ptr(),))
    head = (lg.data_ptr(), C, C, tg.data_ptr(), int(tf), cwd.data_ptr(), 255, N)
    lib.call("hn_seg_loss_fwd" + sfx, *head, HW, int(topk), int(k), *va, ws.data_ptr(), out.data_ptr())
    g = to_dev(np.array([GOUT], np.float32))
    dl = Guarded(M, C)
    lib.call("hn_seg_loss_bwd" + sfx, *head, HW, int(topk), int(k), *va, ws.data_ptr(), g.data_ptr(), dl.ptr(), C)
    res = dict(out=out.cpu().numpy().copy(), d=dl.view.cpu().numpy().reshape(N, HW, C).copy())
    dl.check("dlogits")
    if s2d is not None:
        H, W = s2d
        dz = Guarded(M // 4, ldz, dtype=torch.bfloat16)
        lib.call("hn_seg_loss_bwd_s2d" + sfx, *head, H, W, int(topk), int(k), *va, ws.data_ptr(), g.data_ptr(), dz.ptr(), ldz)
        res["z"] = dz.view.float().cpu().numpy().reshape(N, H // 2, W // 2, ldz).copy()
        dz.check("dz")
    raw = ws.cpu().numpy()
    o = M * 4 + N * 2048 * 4
    res["loss"] = raw[:M * 4].view(np.float32).reshape(N, HW).copy()
    res["state"] = raw[o:o + N * 8].view(np.uint32).reshape(N, 2).copy()
    res["ties"] = raw[o + N * 8:o + N * 12].view(np.uint32).copy()
    return res


def seg_k(loss64, mask):
    """a rank with test_loss_ref_cpu.py's margin (relative gap >= 5e-4 around the k-th largest loss) on the sub-batch"""
    idx = P.labelled(mask)
    k, gap = R.choose_k(loss64[idx] if len(idx) else loss64)
    assert gap >= 5e-4, gap
    return k


@pytest.mark.parametrize("C,tf", [(5, 1), (5, 0), (3, 1)], ids=["vec5_float", "generic5_int64", "generic3_float"])
@pytest.mark.parametrize("n,h,w", SEG_SHAPES)
def test_seg_ce_masked(lib, n, h, w, C, tf):
    logits, target, cw = R.seg_case(0, C, n, h, w)
    loss64, _ = R.seg_ce(logits, target, cw)
    for mask in masks_for(n):
        k = seg_k(loss64, mask)
        for topk in (1, 0):
            what = f"C={C} tf={tf} {(n, h, w)} mask={mask} topk={topk} k={k}"
            r = seg_run(lib, logits, target, cw, tf, topk, k, mask)
            val, grad = P.seg_ce_mean(logits, target, cw, topk, k, mask)
            got = float(r["out"][0])
            print(f"{what}: out {got!r} ref {val!r}")
            assert abs(got - val) <= 1e-5 * abs(val), what
            if not any(mask):
                assert got == 0.0, what
            close(r["d"], grad * GOUT, 1e-4, what + " dlogits")
            for i in range(n):
                if not mask[i]:
                    assert (bits(r["d"][i]) == 0).all(), f"{what}: image {i} is unlabelled and its gradient is not exactly +0.0"
                elif topk:                                             # the selection state of a labelled image: the unmasked contract
                    want = tuple(int(v) for v in R.topk_select(bits(r["loss"][i]), k))
                    assert (int(r["state"][i, 0]), int(r["state"][i, 1]), int(r["ties"][i])) == want, (what, i)
                    assert want[1:] == R.topk_select(loss64[i], k)[1:], (what, i)
            again = seg_run(lib, logits, target, cw, tf, topk, k, mask)
            assert same_bits(again["out"], r["out"]) and same_bits(again["d"], r["d"]), what + ": two runs differ"
            if all(mask):
                u = seg_run(lib, logits, target, cw, tf, topk, k, None)
                assert same_bits(u["out"], r["out"]) and same_bits(u["d"], r["d"]) and same_bits(u["state"], r["state"]), \
                    what + ": the all-ones mask is not the unmasked entry point bit for bit"


@pytest.mark.parametrize("tf", [1, 0], ids=["vec_float", "generic_int64"])
def test_seg_ce_masked_space_to_depth(lib, tf):
    n, h, w, C, ldz = 3, 50, 82, 5, 24
    logits, target, cw = R.seg_case(0, C, n, h, w)
    loss64, _ = R.seg_ce(logits, target, cw)
    for mask in MASKS3:
        k = seg_k(loss64, mask)
        for topk in (1, 0):
            what = f"s2d tf={tf} mask={mask} topk={topk}"
            r = seg_run(lib, logits, target, cw, tf, topk, k, mask, s2d=(h, w), ldz=ldz)
            _, grad = P.seg_ce_mean(logits, target, cw, topk, k, mask)
            want = R.s2d_channels((grad * GOUT).reshape(-1, C), n, h, w, C, ldz)
            z = r["z"]
            assert (z[..., 4 * C:] == 0).all()
            a, b = R.bf16_line(z), R.bf16_line(want)
            frac = float((a != b).mean())
            print(f"{what}: {100 * frac:.4f} % differ, max distance {int(np.abs(a - b).max())} bf16 ulp")
            assert int(np.abs(a - b).max()) <= 1 and frac <= 0.01, what
            for i in range(n):
                if not mask[i]:
                    assert (z[i] == 0).all() and not np.signbit(z[i]).any(), f"{what}: image {i}"
            if all(mask):
                u = seg_run(lib, logits, target, cw, tf, topk, k, None, s2d=(h, w), ldz=ldz)
                assert same_bits(u["z"], z), what


# ------------------------------------------------------------------------------------------------------------------------------------
# focal
# ------------------------------------------------------------------------------------------------------------------------------------
def focal_run(lib, logits, target, cw, tf, gamma, alpha, N, HW, mask):
    C = logits.shape[-1]
    lg = padded_rows(logits.reshape(-1, C), C + 3)
    tg = to_dev(target.reshape(-1).astype(np.float32) if tf else target.reshape(-1))
    cwd = to_dev(cw)
    ws = torch.full((lib.query("hn_seg_loss_blocks", N, HW),), float("nan"), device=dev())
    out = torch.full((1,), float("nan"), device=dev())
    v = None if mask is None else vmask(mask)
    sfx, va = ("", ()) if mask is None else ("_masked", (v.data_ptr(),))
    head = (lg.data_ptr(), C + 3, C, tg.data_ptr(), tf, cwd.data_ptr(), gamma, alpha, N, HW)
    lib.call("hn_seg_focal_fwd" + sfx, *head, *va, ws.data_ptr(), out.data_ptr())
    g = to_dev(np.array([GOUT], np.float32))
    dl = Guarded(N * HW, C, ld=C + 3)
    lib.call("hn_seg_focal_bwd" + sfx, *head, *va, g.data_ptr(), dl.ptr(), C + 3)
    d = dl.view.cpu().numpy().reshape(N, HW, C).copy()
    dl.check("focal dlogits")
    return out.cpu().numpy().copy(), d


@pytest.mark.parametrize("tf", [1, 0])
def test_seg_focal_masked(lib, tf):
    N, HW, C = 3, 4098, 5                                                # two blocks per image
    logits, target, cw = R.focal_case(C, m=N * HW)
    logits, target = logits.reshape(N, HW, C), target.reshape(N, HW)
    for mask in MASKS3:
        val, grad = P.seg_focal(logits, target, cw, 2.0, 1.0, mask)
        out, d = focal_run(lib, logits, target, cw, tf, 2.0, 1.0, N, HW, mask)
        got = float(out[0])
        print(f"focal tf={tf} mask={mask}: out {got!r} ref {val!r}")
        assert abs(got - val) <= 1e-5 * abs(val) and (any(mask) or got == 0.0)
        assert np.isfinite(d).all()
        close(d, grad * GOUT, 1e-4, f"focal dlogits mask={mask}")
        for i in range(N):
            assert mask[i] or (bits(d[i]) == 0).all(), (mask, i)
        out2, d2 = focal_run(lib, logits, target, cw, tf, 2.0, 1.0, N, HW, mask)
        assert same_bits(out, out2) and same_bits(d, d2)
        if all(mask):
            uo, ud = focal_run(lib, logits, target, cw, tf, 2.0, 1.0, N, HW, None)
            assert same_bits(uo, out) and same_bits(ud, d)


# ------------------------------------------------------------------------------------------------------------------------------------
# Lovasz
# ------------------------------------------------------------------------------------------------------------------------------------
def lovasz_run(lib, logits_nhwc, target, mask, s2d):
    n, h, w, c = logits_nhwc.shape
    hw = h * w
    ws = torch.full((lib.query("hn_seg_lovasz_ws_bytes", n, hw, c),), 0xA5, dtype=torch.uint8, device=dev())
    out = torch.full((1,), float("nan"), device=dev())
    v = None if mask is None else vmask(mask)
    sfx, va = ("", ()) if mask is None else ("_masked", (v.data_ptr(),))
    tf = 1 if target.dtype == torch.float32 else 0
    head = (logits_nhwc.data_ptr(), c, c, target.data_ptr(), tf, 255, n)
    lib.call("hn_seg_lovasz_fwd" + sfx, *head, hw, *va, ws.data_ptr(), out.data_ptr())
    g = to_dev(np.array([GOUT], np.float32))
    if s2d:
        dz = Guarded(n * hw // 4, 24, dtype=torch.bfloat16)
        lib.call("hn_seg_lovasz_bwd_s2d" + sfx, *head, h, w, *va, ws.data_ptr(), g.data_ptr(), dz.ptr(), 24)
        d = dz.view.float().cpu().numpy().reshape(n, h // 2, w // 2, 24).copy()
        dz.check("lovasz dz")
    else:
        dl = Guarded(n * hw, c)
        lib.call("hn_seg_lovasz_bwd" + sfx, *head, hw, *va, ws.data_ptr(), g.data_ptr(), dl.ptr(), c)
        d = dl.view.cpu().numpy().reshape(n, h, w, c).copy()
        dl.check("lovasz dlogits")
    return out.cpu().numpy().copy(), d


@pytest.mark.parametrize("tdtype", [torch.float32, torch.int64])
def test_seg_lovasz_masked(lib, tdtype):
    """The margin of these inputs: every pixel's logits are one of 12 palette rows (test_lovasz_gpu.py's tie inputs), so two errors
    |fg - p_c| of a class are either equal bit for bit -- the stable order, pixel index ascending, decides, and with a mask it has to come
    from the remaining pixels -- or differ by more than 1e-4 (asserted), far above what fp32 can reorder.  Continuous random logits have
    neighbours closer than an fp32 ulp at this size; a single swapped pair moves two weights by about 1 / (pixels of the class), which is
    why the unmasked test's 1e-4 bound needs its larger maps."""
    n, c, h, w = 3, 5, 32, 64
    gen = torch.Generator().manual_seed(11)                              # (host generator: the same inputs on every machine)
    palette = torch.randn((12, c), generator=gen) * 2.0
    p64 = torch.softmax(palette.double(), 1)
    for k in range(c):
        vals = torch.unique(torch.cat([p64[:, k], 1.0 - p64[:, k]]))
        assert float((vals[1:] - vals[:-1]).min()) > 1e-4
    x = palette[torch.randint(0, 12, (n, h, w), generator=gen)].contiguous().to(dev())
    t = torch.randint(0, c, (n, h, w), generator=gen).to(dev())
    t[1][t[1] == 3] = 0                                                   # class 3 lives in images 0 and 2 only; class 4 in image 1 only
    t[0][t[0] == 4] = 1
    t[2][t[2] == 4] = 1
    t[:, : h // 4, : w // 3] = 255
    t = t.to(tdtype).contiguous()
    for mask in MASKS3:
        val, grad = P.seg_lovasz(x.permute(0, 3, 1, 2), t, mask)
        grad = np.transpose(grad, (0, 2, 3, 1)) * GOUT
        out, d = lovasz_run(lib, x, t, mask, s2d=False)
        got = float(out[0])
        print(f"lovasz {tdtype} mask={mask}: out {got!r} ref {val!r}")
        assert abs(got - val) <= 1e-5 * abs(val) and (any(mask) or got == 0.0)
        close(d, grad, 1e-4, f"lovasz dlogits mask={mask}")
        for i in range(n):
            assert mask[i] or (bits(d[i]) == 0).all(), (mask, i)
        out2, d2 = lovasz_run(lib, x, t, mask, s2d=False)
        assert same_bits(out, out2) and same_bits(d, d2)
        _, z = lovasz_run(lib, x, t, mask, s2d=True)
        want = R.s2d_channels(grad.reshape(-1, c), n, h, w, c, 24)
        a, b = R.bf16_line(z), R.bf16_line(want)
        assert int(np.abs(a - b).max()) <= 1 and float((a != b).mean()) <= 0.01, mask
        for i in range(n):
            assert mask[i] or (z[i] == 0).all(), (mask, i)
        if all(mask):
            uo, ud = lovasz_run(lib, x, t, None, s2d=False)
            _, uz = lovasz_run(lib, x, t, None, s2d=True)
            assert same_bits(uo, out) and same_bits(ud, d) and same_bits(uz, z)


# ------------------------------------------------------------------------------------------------------------------------------------
# detection
# ------------------------------------------------------------------------------------------------------------------------------------
KIND_ID = {"giou": 1, "diou": 2, "ciou": 3}
DET_KINDS = ("smooth_l1", "giou", "diou", "ciou")


def det_run(lib, cls, reg, anc, ann, kind, mask, given=None, gout=(1.0, 50.0)):
    """hn_det_loss[_iou]_fwd[_assigned](_masked) + _bwd(_masked) -> everything they write; given: an int16 [N, A] assignment to read"""
    N, A, Kc = cls.shape
    Mx = ann.shape[1]
    iou = kind != "smooth_l1"
    c, r, a, b = to_dev(np.asarray(cls, np.float32)), to_dev(np.asarray(reg, np.float32)), to_dev(np.asarray(anc, np.float32)), \
        to_dev(np.asarray(ann, np.float32))
    blocks = lib.query("hn_det_loss_blocks", A)
    cols = 4 if iou else 3
    assign = torch.full((N, A), -7, dtype=torch.int16, device=dev()) if given is None else \
        torch.from_numpy(np.asarray(given, np.int16)).to(dev()).contiguous()
    before = assign.clone()
    part = torch.full((N, blocks, cols), float("nan"), device=dev())
    npos = torch.full((N,), float("nan"), device=dev())
    out = torch.full((cols - 1,), float("nan"), device=dev())
    v = None if mask is None else vmask(mask)
    sfx, va = ("", ()) if mask is None else ("_masked", (v.data_ptr(),))
    base = "hn_det_loss_iou" if iou else "hn_det_loss"
    extra = (KIND_ID[kind],) if iou else ()
    head = (c.data_ptr(), r.data_ptr(), a.data_ptr(), b.data_ptr(), N, A, Kc, Mx, *extra, *va)
    lib.call(base + ("_fwd" if given is None else "_fwd_assigned") + sfx, *head, assign.data_ptr(), part.data_ptr(), npos.data_ptr(), out.data_ptr())
    g = to_dev(np.array(gout, np.float32))
    dcls, dreg = Guarded(N * A, Kc), Guarded(N * A, 4)
    lib.call(base + "_bwd" + sfx, *head, assign.data_ptr(), npos.data_ptr(), g.data_ptr(), dcls.ptr(), dreg.ptr())
    res = dict(out=out.cpu().numpy().copy(), npos=npos.cpu().numpy().copy(), assign=assign.cpu().numpy().astype(np.int64),
               dcls=dcls.view.cpu().numpy().reshape(N, A, Kc).copy(), dreg=dreg.view.cpu().numpy().reshape(N, A, 4).copy())
    dcls.check("dcls")
    dreg.check("dreg")
    if given is not None:
        assert torch.equal(assign, before), "a given assignment was written"
    return res


def det_check(lib, cls, reg, anc, ann, kind, mask, given, what, grads=True, gout=(1.0, 50.0)):
    N = cls.shape[0]
    ref = P.det(cls, reg, anc, ann, mask, kind, assign=given, gcls=gout[0], greg=gout[1])
    got = det_run(lib, cls, reg, anc, ann, kind, mask, given, gout)
    names = ("cls", "reg") + (("pos_iou",) if kind != "smooth_l1" else ())
    print(f"{what}: " + "  ".join(f"{nm} {float(got['out'][i])!r} / {ref[nm]!r}" for i, nm in enumerate(names)) + f"  npos {ref['npos']}")
    for i, nm in enumerate(names):
        assert abs(float(got["out"][i]) - ref[nm]) <= 2e-5 * max(abs(ref[nm]), 1e-6), (what, nm, float(got["out"][i]), ref[nm])
        assert any(mask) or float(got["out"][i]) == 0.0, (what, nm)
    assert got["npos"].tolist() == [float(v) for v in ref["npos"]], what
    if given is None:
        assert (got["assign"] == ref["assign"]).all(), what
    assert np.isfinite(got["dcls"]).all() and np.isfinite(got["dreg"]).all()
    if grads:
        close(got["dcls"], ref["dcls"], 2e-4, what + " dcls")
        close(got["dreg"], ref["dreg"], 2e-4, what + " dreg")
    for n in range(N):
        if not mask[n]:
            assert (bits(got["dcls"][n]) == 0).all() and (bits(got["dreg"][n]) == 0).all(), f"{what}: image {n} is unlabelled"
            assert given is not None or (got["assign"][n] == -2).all(), f"{what}: image {n}'s assign row is not -2 throughout"
    again = det_run(lib, cls, reg, anc, ann, kind, mask, given, gout)
    assert all(same_bits(again[k], got[k]) for k in got), what + ": two runs differ"
    if all(mask):
        u = det_run(lib, cls, reg, anc, ann, kind, None, given, gout)
        assert all(same_bits(u[k], got[k]) for k in got), what + ": the all-ones mask is not the unmasked entry point bit for bit"
    return got, ref


def no_ignore_zone(anc, ann):
    """a given assignment in ATSS's value range (index or -1): the max-IoU one with its ignored anchors turned into background"""
    a = P.max_iou_assign(anc, ann)
    return np.where(a == -2, -1, a).astype(np.int16)


@pytest.fixture(scope="module")
def kats():
    z = load_npz("loss_kats.npz")
    cls = np.clip(z["det/cls"] * 4.5, 0, 1).astype(np.float32)            # spread over (0, 0.9]: both focal branches and the clamp
    cls[0, :50] = 0.0
    cls[0, 50:100] = 1.0
    return dict(cls=cls, reg=z["det/reg"].astype(np.float32), anc=z["det/anchors"].reshape(-1, 4).astype(np.float32),
                ann=z["det/ann"].astype(np.float32))


@pytest.mark.parametrize("kind", DET_KINDS)
def test_det_masked_recorded_inputs(lib, K, kats, kind):
    """3 images, 6 138 anchors, 71 / 35 / 0 positives: own assignment and the device's ATSS assignment handed in"""
    from tests.test_det_atss_cpu import DET
    c, r, a, b = kats["cls"], kats["reg"], kats["anc"], kats["ann"]
    assert a.shape[0] == 6138
    _, sizes = det_atss_ref.make_anchors(128, 256, DET)
    atss, _ = K.det_atss_assign(torch.from_numpy(a).to(dev()), sizes, torch.from_numpy(b).to(dev()))
    atss = atss.cpu().numpy()
    assert int((atss[0] >= 0).sum()) > 71 and not (atss == -2).any()
    for mask in MASKS3:
        got, ref = det_check(lib, c, r, a, b, kind, mask, None, f"{kind} recorded mask={mask}")
        assert ref["npos"] == [71 * mask[0], 35 * mask[1], 0]
        det_check(lib, c, r, a, b, kind, mask, atss, f"{kind} recorded atss mask={mask}")


@pytest.mark.parametrize("Kc", [1, 9])
@pytest.mark.parametrize("A", [255, 256, 257])
def test_det_masked_tail_shapes(lib, A, Kc):
    from tests.test_det_iou_gpu import tail_case
    cls, reg, anc, ann, _ = tail_case(A, Kc)
    cls, reg, anc, ann = cls.numpy(), reg.numpy(), anc[0].numpy(), ann.numpy()
    given = no_ignore_zone(anc, ann)
    for kind in DET_KINDS:
        for mask in MASKS3:
            _, ref = det_check(lib, cls, reg, anc, ann, kind, mask, None, f"{kind} A={A} K={Kc} mask={mask}", gout=(1.0, 1.0))
            assert kind == "smooth_l1" or not any(mask) or ref["margin"] > 1e-3
            det_check(lib, cls, reg, anc, ann, kind, mask, given, f"{kind} A={A} K={Kc} given mask={mask}", gout=(1.0, 1.0))


@pytest.mark.parametrize("kind", DET_KINDS)
def test_det_masked_17_images(lib, kind):
    """N = 17: the finalize walks 16 images per pass; labelled images on both sides, and image 1 (no boxes in det_case) unlabelled"""
    N, A, Kc = 17, 257, 9
    cls, reg, anc, ann = R.det_case(N, A, Kc)
    for mask in masks_for(17):
        det_check(lib, cls, reg, anc, ann, kind, mask, None, f"{kind} N=17 mask={''.join(map(str, mask))}")
    det_check(lib, cls, reg, anc, ann, kind, MASK17, no_ignore_zone(anc, ann), f"{kind} N=17 given")


# ------------------------------------------------------------------------------------------------------------------------------------
# lane
# ------------------------------------------------------------------------------------------------------------------------------------
def lane_run(lib, z, t, ratio, rows, mask, offset=0, alpha=10.0, gpos=1.3, gneg=0.7):
    M = z.shape[0]
    zd, td = to_dev(z, offset), to_dev(t)
    lsm = torch.full((M, 2), float("nan"), device=dev())
    pmask = torch.full((M,), 0x5A, dtype=torch.uint8, device=dev())
    out, aux = torch.full((2,), float("nan"), device=dev()), torch.full((4,), float("nan"), device=dev())
    gp, gn = to_dev(np.array([gpos], np.float32)), to_dev(np.array([gneg], np.float32))
    dz = Guarded(M, 2)
    if mask is None:
        lib.call("hn_lane_cls_loss_fwd", zd.data_ptr(), td.data_ptr(), M, float(ratio), float(alpha), lsm.data_ptr(), pmask.data_ptr(),
                 out.data_ptr(), aux.data_ptr())
        lib.call("hn_lane_cls_loss_bwd", lsm.data_ptr(), pmask.data_ptr(), aux.data_ptr(), gp.data_ptr(), gn.data_ptr(), float(alpha), M, dz.ptr())
    else:
        v = vmask(mask)
        lib.call("hn_lane_cls_loss_fwd_masked", zd.data_ptr(), td.data_ptr(), M, rows, v.data_ptr(), float(ratio), float(alpha), lsm.data_ptr(),
                 pmask.data_ptr(), out.data_ptr(), aux.data_ptr())
        lib.call("hn_lane_cls_loss_bwd_masked", lsm.data_ptr(), pmask.data_ptr(), aux.data_ptr(), gp.data_ptr(), gn.data_ptr(), float(alpha), M,
                 rows, v.data_ptr(), dz.ptr())
    res = dict(lsm=lsm.cpu().numpy(), pmask=pmask.cpu().numpy(), out=out.cpu().numpy(), aux=aux.cpu().numpy(), dlogits=dz.view.cpu().numpy().copy())
    dz.check("lane dlogits")
    return res, (pmask, aux)


def lane_loc_run(lib, p, t, pmask_dev, aux_dev, wcol, gout=1.7):
    M, L = p.shape
    pd, td = to_dev(p), to_dev(t)
    rowloss, rownorm = Guarded(1, M), Guarded(1, M)
    out = torch.full((1,), float("nan"), device=dev())
    lib.call("hn_lane_loc_loss_fwd", pd.data_ptr(), td.data_ptr(), pmask_dev.data_ptr(), aux_dev.data_ptr(), M, L, wcol, 10.0, rowloss.ptr(),
             rownorm.ptr(), out.data_ptr())
    g = to_dev(np.array([gout], np.float32))
    dp = Guarded(M, L)
    lib.call("hn_lane_loc_loss_bwd", pd.data_ptr(), td.data_ptr(), pmask_dev.data_ptr(), rownorm.ptr(), aux_dev.data_ptr(), g.data_ptr(), M, L,
             wcol, 10.0, dp.ptr())
    d = dp.view.cpu().numpy().copy()
    dp.check("dpred")
    return float(out.cpu()[0]), d


def lane_case(M, seed):
    """random rows: ~4 % positives, logits randn * 2 (fp32): distinct log-probs, no ties at the OHEM rank"""
    g = np.random.default_rng(seed)
    z = (g.standard_normal((M, 2)) * 2).astype(np.float32)
    pos = g.random(M) < 0.04
    t = np.stack([~pos, pos], 1).astype(np.float32)
    return z, t


@pytest.mark.parametrize("rows,offset", [(128, 0), (2731, 0), (10923, 0), (128, 1)], ids=["reg8", "reg32", "global", "off_alignment"])
def test_lane_masked(lib, rows, offset):
    """M = 3 * 128 (reg<8>), 3 * 2731 = 8193 (reg<32>), 3 * 10923 = 32769 (global-memory kernel); logits 4 bytes off alignment: the
    global-memory kernel at M = 384"""
    N = 3
    M = N * rows
    z, t = lane_case(M, rows)
    L, wcol = 12, 10
    g = np.random.default_rng(rows + 1)
    lt = ((g.integers(-40, 41, (M, L)) / 8.0) * (g.random((M, L)) < 0.7)).astype(np.float32)
    lp = (lt + g.standard_normal((M, L)) * 1.5).astype(np.float32)
    for mask in MASKS3:
        what = f"lane rows={rows} offset={offset} mask={mask}"
        got, (pm_dev, aux_dev) = lane_run(lib, z, t, 15.0, rows, mask, offset)
        ref = P.lane_cls(z, t, rows, mask, 15.0, 10.0, gpos=1.3, gneg=0.7)
        assert (got["pmask"] == ref["pmask"]).all(), what
        assert [float(v) for v in got["aux"][1:]] == [float(ref["posn"]), float(ref["npos"]), float(ref["nneg"])], (what, got["aux"])
        lsm64 = R.lane_cls(z, t)["lsm"]
        close(got["lsm"], lsm64, 2e-5, what + " lsm", floor=1.0)          # written for every row, labelled or not
        thr = P.lane_select(got["lsm"][:, 0], rows, mask, ref["pmask"], ref["k"])
        assert bits(got["aux"][0]) == bits(thr), f"{what}: threshold {got['aux'][0]!r} != {thr!r} (rank {ref['k']} of {ref['nneg']})"
        for i, nm in enumerate(("pos", "neg")):
            assert abs(float(got["out"][i]) - ref[nm]) <= 2e-5 * max(abs(ref[nm]), 1.0), (what, nm, float(got["out"][i]), ref[nm])
            assert any(mask) or float(got["out"][i]) == 0.0
        close(got["dlogits"], ref["dlogits"], 2e-5, what + " dlogits", floor=1.0)
        dead = np.ones(M, bool)
        dead[ref["rows"]] = False
        assert (bits(got["dlogits"][dead]) == 0).all(), what + ": an unlabelled row has a gradient"
        # the location loss follows through pmask and aux
        val, grad = P.lane_loc(lp, lt, rows, mask, ref["pmask"], ref["posn"], wcol, gout=1.7)
        loc, dp = lane_loc_run(lib, lp, lt, pm_dev, aux_dev, wcol)
        assert abs(loc - val) <= 2e-5 * max(abs(val), 1.0) and (any(mask) or loc == 0.0), (what, loc, val)
        close(dp, grad, 2e-5, what + " dpred", floor=1.0)
        assert (bits(dp[dead]) == 0).all(), what
        again, _ = lane_run(lib, z, t, 15.0, rows, mask, offset)
        assert all(same_bits(again[k], got[k]) for k in got), what + ": two runs differ"
        if all(mask):
            u, _ = lane_run(lib, z, t, 15.0, rows, None, offset)
            assert all(same_bits(u[k], got[k]) for k in got), what + ": the all-ones mask is not the unmasked entry point bit for bit"


# ------------------------------------------------------------------------------------------------------------------------------------
# capture: one graph, three mask contents
# ------------------------------------------------------------------------------------------------------------------------------------
def test_one_captured_graph_serves_every_mask(K):
    N, h, w, C = 3, 16, 24, 5
    logits, target, cw = R.seg_case(0, C, N, h, w)
    seg = torch.from_numpy(logits.reshape(N, h, w, C)).to(dev()).permute(0, 3, 1, 2).requires_grad_(True)
    tgt = torch.from_numpy(target.reshape(N, h, w)).float().to(dev())
    cwd = torch.from_numpy(cw).to(dev())
    cls, reg, anc, ann = (torch.from_numpy(v).to(dev()) for v in R.det_case(N, 257, 9))
    cls.requires_grad_(True)
    reg.requires_grad_(True)
    rows = 128
    z, t = lane_case(N * rows, 3)
    lz = torch.from_numpy(z).to(dev()).view(N, rows, 2).requires_grad_(True)
    lt = torch.from_numpy(t).to(dev()).view(N, rows, 2)
    g = np.random.default_rng(9)
    loc_t = torch.from_numpy(((g.integers(-40, 41, (N, rows, 12)) / 8.0) * (g.random((N, rows, 12)) < 0.7)).astype(np.float32)).to(dev())
    loc_p = (loc_t + 0.7).clone().requires_grad_(True)
    tv = torch.ones((3, N), dtype=torch.uint8, device=dev())
    leaves = (seg, cls, reg, lz, loc_p)

    def step():
        ls = K.seg_loss_hip(seg, tgt, cwd, True, 0.3, valid=tv[0])
        lc, lr, iou = K.det_iou_loss_hip(cls, reg, anc, ann, "ciou", valid=tv[1])
        pos, neg, pmask, aux = K.lane_cls_loss_hip(lt, lz, valid=tv[2], rows_per_image=rows)
        loc = K.lane_loc_loss_hip(pmask, aux, loc_t, loc_p, points_per_line=10, valid=tv[2], rows_per_image=rows)
        losses = (ls.reshape(1), lc, lr, pos.reshape(1), neg.reshape(1), loc.reshape(1))
        grads = torch.autograd.grad(torch.cat(losses).sum(), leaves)
        return losses + (iou,) + grads

    contents = (torch.tensor([[1, 0, 1], [0, 1, 1], [1, 1, 0]]), torch.tensor([[0, 0, 1], [1, 0, 0], [0, 0, 0]]),
                torch.tensor([[1, 1, 1], [1, 1, 1], [1, 1, 1]]))
    eager = []
    for c in contents:
        tv.copy_(c.to(torch.uint8))
        eager.append([o.detach().clone() for o in step()])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    tv.fill_(1)
    with torch.cuda.graph(graph):
        static = step()
    for c, want in zip(contents, eager):
        tv.copy_(c.to(torch.uint8))
        graph.replay()
        torch.cuda.synchronize()
        for i, (a, b) in enumerate(zip(static, want)):
            assert same_bits(a.detach().cpu().numpy(), b.cpu().numpy()), (c.tolist(), i)
    assert float(eager[1][3]) == 0.0 and float(eager[1][4]) == 0.0 and float(eager[1][5]) == 0.0     # lane row 000
    assert bool((eager[1][-2] == 0).all()) and bool((eager[0][-5][1] == 0).all())


# ------------------------------------------------------------------------------------------------------------------------------------
# module and trainer
# ------------------------------------------------------------------------------------------------------------------------------------
def tiny(cfg_edit=None):
    from multitask_hydranet_amd import HydraNet
    z = load_npz("tiny_hydranet.npz")
    cfgs = load_cfg("hydranet_tiny.yml")
    if cfg_edit:
        cfg_edit(cfgs)
    net = HydraNet(copy.deepcopy(cfgs))
    net.load_state_dict(tiny_state(z))
    net = net.to(dev()).train()
    net.lane_points_per_line = int(z["meta/lane_points_per_line"])
    batch = {k[3:]: torch.from_numpy(z[k].copy()) for k in z.files if k.startswith("in/")}
    return z, cfgs, net, batch


def set_det(kind, assigner):
    def edit(cfgs):
        cfgs["detection"]["loss_reg_type"] = kind
        cfgs["detection"]["assigner"] = assigner
    return edit


@pytest.mark.parametrize("kind,assigner", [("smooth_l1", "max_iou"), ("ciou", "atss")])
def test_cal_loss_passes_the_rows_to_the_ops(K, kind, assigner):
    _, _, net, batch = tiny(set_det(kind, assigner))
    gb = {k: v.to(dev()) for k, v in batch.items()}
    gb["image"], gb["gt_seg"] = gb["image"].float(), gb["gt_seg"].float()
    n = gb["image"].shape[0]
    assert n == 2
    tv = torch.tensor([[0, 1], [1, 0], [1, 1]], dtype=torch.uint8, device=dev())
    out = net(gb["image"])
    net._seg_grad_slot = None                   # the seg gradient as an fp32 dlogits tensor (not handed over in operand form): seg.grad
    seg = out["seg"]
    seg.retain_grad()
    ld = net.cal_loss(out, dict(gb, task_valid=tv))
    d = out["detection"]
    use_top_k, ratio, use_focal = net._seg_cfg
    with torch.no_grad():
        want_seg = K.seg_focal_loss_hip(seg, gb["gt_seg"], net._seg_class_weight, valid=tv[0]) if use_focal else \
            K.seg_loss_hip(seg, gb["gt_seg"], net._seg_class_weight, use_top_k, ratio, valid=tv[0])
        if assigner == "atss":
            h, w = net._anchor_hw(d["anchors"])
            assign, _ = K.det_atss_assign(d["anchors"], net.anchor_level_sizes(h, w), gb["gt_det"], net.atss_topk, net.anchors_per_location)
            cl, rl, iou = K.det_iou_loss_hip(d["classification"], d["regression"], d["anchors"], gb["gt_det"], kind, assign=assign, valid=tv[1])
            assert same_bits(net.det_pos_iou.cpu().numpy(), iou.reshape(()).cpu().numpy())
        else:
            cl, rl = K.det_loss_hip(d["classification"], d["regression"], d["anchors"], gb["gt_det"], valid=tv[1])
        pc = out["lane"]["predict_cls"]
        rows = pc.numel() // 2 // n
        pos, neg, pmask, aux = K.lane_cls_loss_hip(gb["gt_cls"], pc, valid=tv[2], rows_per_image=rows)
        loc = K.lane_loc_loss_hip(pmask, aux, gb["gt_loc"], out["lane"]["predict_loc"], points_per_line=net.lane_points_per_line)
    want = dict(loss_seg=want_seg, loss_det_cls=cl, loss_det_reg=rl, loss_lane_cls_pos=pos, loss_lane_cls_neg=neg, loss_lane_loc=loc)
    assert set(ld) == set(want)
    for k in want:
        assert same_bits(ld[k].detach().cpu().numpy().reshape(-1), want[k].cpu().numpy().reshape(-1)), k
    # the masked det loss is the one-image loss of image 0, the masked seg loss that of image 1
    with torch.no_grad():
        if assigner == "max_iou":
            c1, r1 = K.det_loss_hip(d["classification"][:1], d["regression"][:1], d["anchors"], gb["gt_det"][:1])
            assert abs(float(c1) - float(cl)) <= 2e-5 * abs(float(c1)) and abs(float(r1) - float(rl)) <= 2e-5 * max(abs(float(r1)), 1e-6)
    net.total_loss(ld).backward()
    assert bool((seg.grad[0] == 0).all()) and bool((seg.grad[1] != 0).any())
    with pytest.raises(ValueError, match="task_valid"):
        net.cal_loss(net(gb["image"]), dict(gb, task_valid=tv.cpu()))
    net.check_finite = True                                               # a task without a labelled image: loss 0 is no divergence
    ld0 = net.cal_loss(net(gb["image"]), dict(gb, task_valid=torch.zeros_like(tv)))
    assert all(float(v.detach()) == 0.0 for v in ld0.values())


@pytest.mark.parametrize("capture", [False, True], ids=["eager", "captured"])
def test_train_step_with_a_changing_mask(K, capture):
    from multitask_hydranet_amd.train import HydraTrainer
    z = load_npz("tiny_hydranet.npz")
    cfgs = load_cfg("hydranet_tiny.yml")
    cfgs["train"].update(dict(continue_train=False, weight_file="", epoch=1, lr=1e-4, weight_decay=0.0))
    batch = {k[3:]: torch.from_numpy(z[k].copy()) for k in z.files if k.startswith("in/")}
    masks = ([[1, 1], [1, 1], [1, 1]], [[0, 1], [1, 0], [1, 1]], [[0, 0], [0, 1], [1, 0]], [[1, 0], [0, 0], [0, 0]], [[0, 1], [1, 0], [1, 1]])
    tr = HydraTrainer(copy.deepcopy(cfgs), trainloader=[batch], validloader=None, iters_per_epoch=len(masks), capture_step=capture)
    tr.hydranet.load_state_dict(tiny_state(z))
    tr.hydranet.lane_points_per_line = int(z["meta/lane_points_per_line"])
    tr.hydranet.check_finite = True
    seen, graphs = [], set()
    for m in masks:
        b = {k: v.clone() for k, v in batch.items()}
        b["task_valid"] = torch.tensor(m, dtype=torch.uint8)
        ld = tr.train_step(b)
        seen.append({k: float(v.detach()) for k, v in ld.items()})
        if tr._cap is not None:
            graphs.add(id(tr._cap[1]))
    assert (tr._cap is not None) == capture and len(graphs) == (1 if capture else 0)      # one graph serves every mask
    assert all(np.isfinite(list(s.values())).all() for s in seen)
    assert seen[2]["loss_seg"] == 0.0 and seen[3]["loss_det_cls"] == 0.0 and seen[3]["loss_lane_cls_pos"] == 0.0 and seen[3]["loss_seg"] > 0
    assert seen[1]["loss_seg"] > 0 and seen[1]["loss_seg"] != seen[0]["loss_seg"]


def test_valid_scores_labelled_images_only(K):
    from multitask_hydranet_amd import lane_metric as LM
    from multitask_hydranet_amd.lane_codec import LaneCodec
    from multitask_hydranet_amd.train import HydraTrainer
    z = load_npz("tiny_hydranet.npz")
    cfgs = load_cfg("hydranet_tiny.yml")
    cfgs["train"].update(dict(continue_train=False, weight_file="", epoch=1, lr=1e-4, weight_decay=0.0))
    cfgs["lane"]["conf_thres"] = 0.3
    batch = {k[3:]: torch.from_numpy(z[k].copy()) for k in z.files if k.startswith("in/")}
    n = batch["image"].shape[0]
    hh, ww = batch["image"].shape[2], batch["image"].shape[3]
    shapes = [{"width": 1920, "height": 1080}] * n
    coder = LaneCodec(ww, hh, cfgs["lane"]["anchor_stride"], hh // cfgs["lane"]["interval"])
    sd = tiny_state(z)

    def trainer(loader):
        tr = HydraTrainer(copy.deepcopy(cfgs), trainloader=[dict(batch)], validloader=loader, iters_per_epoch=1)
        tr.hydranet.load_state_dict(sd)
        tr.hydranet.lane_points_per_line = int(z["meta/lane_points_per_line"])
        return tr
    # as tests/test_lane_metric_batch_gpu.py: shift the lane head's biases so that the tiny model predicts lanes with points
    tr = trainer([])
    net = tr.hydranet.eval()
    with torch.no_grad():
        logits = net(batch["image"].to(tr.device).float())["lane"]["predict_cls"].float()
    margin = (logits[..., 0] - logits[..., 1]).flatten()
    sd["laneheader.conv_cls_conv.3.bias"] = sd["laneheader.conv_cls_conv.3.bias"].clone()
    sd["laneheader.conv_cls_conv.3.bias"][1] += float(torch.quantile(margin, 0.8))
    ppl = int(z["meta/lane_points_per_line"])
    for name, k in (("laneheader.conv_down_conv.3.bias", ppl), ("laneheader.conv_up_conv.3.bias", 0)):
        sd[name] = sd[name].clone()
        sd[name][k] += 6.0
    gts = [{"Lines": [[{"x": 100.0 + 30 * k + 200 * i, "y": 1000.0 - 80 * k} for k in range(6)]], "Labels": [1]} for i in range(n)]
    plain = [dict(batch, src_image_shape=shapes, gt_lane_json=gts) for _ in range(2)]
    tv = [torch.tensor([[1, 0], [0, 1], [1, 0]], dtype=torch.uint8), torch.tensor([[0, 0], [1, 1], [0, 1]], dtype=torch.uint8)]
    masked = [dict(b, task_valid=m) for b, m in zip(plain, tv)]
    full = trainer(plain)
    full.valid(0, lane_coder=coder, det_conf_thres=0.05)
    part = trainer(masked)
    part.valid(0, lane_coder=coder, det_conf_thres=0.05)
    # mIoU: one labelled image over the two batches
    px = batch["gt_seg"][0].numel()
    assert int(full.metric_evaluator_iou.conf.sum()) == 2 * n * px and int(part.metric_evaluator_iou.conf.sum()) == px
    one = trainer([dict(plain[0], task_valid=torch.tensor([[1, 0], [1, 1], [1, 1]], dtype=torch.uint8))])
    one.valid(0, lane_coder=coder, det_conf_thres=0.05)
    assert torch.equal(one.metric_evaluator_iou.conf, part.metric_evaluator_iou.conf)
    # COCO records: the labelled images' records, under their own ids (batch_size_valid ids per batch)
    bs = cfgs["train"].get("batch_size_valid", n)
    ids = {it * bs + 1 + i for it, m in enumerate(tv) for i in range(n) if int(m[1, i])}
    all_ids = {r["image_id"] for r in full.last_valid["detect_result"]}
    assert all_ids - ids, "the tiny model has no detection on an unlabelled image at this threshold: the check would be empty"
    assert part.last_valid["detect_result"] == [r for r in full.last_valid["detect_result"] if r["image_id"] in ids]
    # lane F1: the labelled images' pairs
    keep = [bool(int(m[2, i])) for m in tv for i in range(n)]
    lr_ = part.last_valid["lane_result"]
    assert len(lr_) == 2 * n
    pairs = [dict(pr_result=r["pr_result"], gt_result={**g, "Shape": r["pr_result"]["Shape"]}) for r, g, on in zip(lr_, gts + gts, keep) if on]
    ref = LM.LaneMetric(method="f1_measure", iou_thresh=0.5, lane_width=30, thresh_list=[0.5])
    ref(output=pairs)
    assert part.last_valid["lane_f1"] == ref.summary()
    assert sum(r["gt_num"] for r in ref.metric_handlers[0].result_record) == sum(keep)
    # the validation losses are masked like training
    assert part.last_valid["losses"][1]["loss_seg"] == 0.0 and part.last_valid["losses"][0]["loss_seg"] > 0
    assert part.last_valid["losses"][0]["loss_seg"] != full.last_valid["losses"][0]["loss_seg"]
