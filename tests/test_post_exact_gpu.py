"""The kernels of csrc/hn_post.hip other than the detection NMS -- lane decode + lane NMS, input pre-processing, the seg confusion counts,
the seg overlay, the lane rasteriser and its pair counts -- held to the numpy restatements of tests/post_ref.py through the C entry
points, on the cases of tests/post_cases.py (tests/test_post_ref_cpu.py holds those restatements to the oracle on the same cases and
shows which case would notice which fault).

Every output lies between sentinel guard bands (tests/guards.py: Guarded for the 32-bit outputs, GuardedBytes for uint8 / uint64) and
is compared with ==.  The lane x coordinates are integers times a float32 interval, added to an integer centre with separately rounded
operations on both sides, so they are bit-equal too.  The one tolerance is the lane probability: the device expf and torch's softmax
differ in the last place, bound rtol = 2e-6 as in test_post_gpu.py::_check_lanes (the decisions taken on it are exact: the cases keep
every probability tied or 1e-3 apart, and on the threshold or 1e-3 from it)."""
import numpy as np
import pytest
import torch

from tests import post_cases as Cs
from tests import post_ref as R
from tests.guards import SENT32, Guarded, GuardedBytes, dev

pytestmark = pytest.mark.gpu

HN_ERR_ARG, HN_ERR_UNSUPPORTED = 1, 3
SENT_I32 = SENT32                                           # the sentinel read as int32
PROB_RTOL = 2e-6


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    import __graft_entry__ as g
    g.build()
    from multitask_hydranet_amd._lib import lib
    return lib()


def D(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def rc_of(L, name, *args):
    """the entry point's status (lib().call raises on a non-zero one)"""
    return L.raw(name)(*args, torch.cuda.current_stream().cuda_stream)


def i32(g):
    return g.view.contiguous().view(torch.int32).cpu().numpy()


def untouched(g):
    return bool((g.buf.view(torch.int32) == SENT_I32).all())


# =====================================================================================================================================
# lane decode + lane NMS
# =====================================================================================================================================
def lane_outputs(n, hw, ppl):
    return dict(X=Guarded(n * hw, ppl), prob=Guarded(n, hw), start=Guarded(n, hw), end=Guarded(n, hw), order=Guarded(n, hw), keep=Guarded(n, hw),
                counts=Guarded(1, n))


def lane_launch(L, c, out):
    W, H, stride, ppl = c["geometry"]
    cls, loc = D(c["cls"]), D(c["loc"])
    rc = rc_of(L, "hn_lane_decode_nms", cls.data_ptr(), loc.data_ptr(), c["cls"].shape[0], W, H, stride, ppl, c["thr"], c["nms_thr"], c["use_mean"],
               c["margin"], *[out[k].ptr() for k in ("X", "prob", "start", "end", "order", "keep", "counts")])
    torch.cuda.synchronize()
    return rc


def lane_check(L, name, c):
    W, H, stride, ppl = c["geometry"]
    n, hw = c["cls"].shape[:2]
    out = lane_outputs(n, hw, ppl)
    assert lane_launch(L, c, out) == 0
    for k, g in out.items():
        g.check(f"hn_lane_decode_nms {name} {k}")
    r = R.lane_decode_nms(c["cls"], c["loc"], c["geometry"], c["thr"], c["nms_thr"], c["use_mean"], c["margin"])
    prob = out["prob"].view.cpu().numpy()
    worst = float(np.max(np.abs(prob - r["prob"]) / r["prob"]))
    print(f"hn_lane_decode_nms {name}: worst relative prob error {worst:.3e}")
    np.testing.assert_allclose(prob, r["prob"], rtol=PROB_RTOL, atol=0)
    eq = c["cls"][..., 0] == c["cls"][..., 1]
    assert np.array_equal(prob[eq], r["prob"][eq])                                          # equal logits: exactly 0.5
    for k in ("start", "end"):
        got = i32(out[k])
        bad = np.argwhere(got != r[k])
        assert not len(bad), f"{name}: {k} differs at (image, anchor) {bad[:6].tolist()}: got {got[tuple(bad[0])]} want {r[k][tuple(bad[0])]}"
    xbits = i32(out["X"]).reshape(n, hw, ppl)
    x = out["X"].view.cpu().numpy().reshape(n, hw, ppl)
    w = r["written"]
    bad = np.argwhere(w & (x != r["X"]))
    assert not len(bad), f"{name}: X differs at (image, anchor, position) {bad[:6].tolist()}: got {x[tuple(bad[0])]!r} want {r['X'][tuple(bad[0])]!r}"
    bad = np.argwhere(~w & (xbits != SENT_I32))
    assert not len(bad), f"{name}: X written outside start <= p < end at (image, anchor, position) {bad[:6].tolist()}"
    counts = i32(out["counts"]).reshape(n)
    assert counts.tolist() == r["count"].tolist(), f"{name}: counts {counts.tolist()} want {r['count'].tolist()}"
    order, keep = i32(out["order"]), i32(out["keep"])
    for i in range(n):
        cnt = int(counts[i])
        assert order[i, :cnt].tolist() == r["order"][i].tolist(), f"{name}: order of image {i}"
        assert keep[i, :cnt].tolist() == r["keep"][i].tolist(), f"{name}: keep of image {i} (order {r['order'][i].tolist()})"
        assert bool((order[i, cnt:] == SENT_I32).all()) and bool((keep[i, cnt:] == SENT_I32).all()), f"{name}: order / keep written beyond count"
    return r, counts


CONTENT = Cs.lane_content_cases()


@pytest.mark.parametrize("name", list(CONTENT))
def test_lane_content(L, name):
    r, counts = lane_check(L, name, CONTENT[name])
    assert counts[1] == 0 and counts[2] == 32                                               # the empty image and the full one of the batch


@pytest.mark.parametrize("geom", Cs.GEOMETRIES, ids=[g[0] for g in Cs.GEOMETRIES])
def test_lane_geometry(L, geom):
    c = Cs.lane_geometry_case(*geom)
    r, counts = lane_check(L, geom[0], c)
    for i in range(2):
        assert set(c["planted"]) <= set(r["order"][i].tolist())


def test_lane_geometry_above_the_cap_is_refused(L):
    """7232 anchors need more LDS than the kernel may ask for: HN_ERR_UNSUPPORTED, nothing written, and the wrapper raises"""
    from multitask_hydranet_amd import lane_codec as LC
    from multitask_hydranet_amd._lib import HipKernelError
    name, fw, fh, ppl = Cs.REFUSED_GEOMETRY
    c = Cs.lane_geometry_case(name, fw, fh, ppl)
    n, hw = c["cls"].shape[:2]
    assert hw == 7232 and c["loc"].shape[2] == 34
    out = lane_outputs(n, hw, ppl)
    assert lane_launch(L, c, out) == HN_ERR_UNSUPPORTED
    for k, g in out.items():
        assert untouched(g), f"hn_lane_decode_nms refused the shape but wrote {k}"
    W, H, stride, _ = c["geometry"]
    with pytest.raises(HipKernelError):
        LC.decode_batch(D(c["cls"]), D(c["loc"]), LC.LaneCodec(W, H, stride, ppl), 0.5, 40.0, False)


# =====================================================================================================================================
# pre-processing
# =====================================================================================================================================
@pytest.mark.parametrize("case", Cs.PREPROCESS_SHAPES, ids=[c[0] for c in Cs.PREPROCESS_SHAPES])
def test_preprocess(L, case):
    name, n, (hs, ws), (hd, wd) = case
    frames = Cs.preprocess_case(*case)
    src = D(frames)
    dst = Guarded(n * 3, hd * wd)
    assert rc_of(L, "hn_preprocess_bgr", src.data_ptr(), n, hs, ws, dst.ptr(), hd, wd) == 0
    torch.cuda.synchronize()
    dst.check(f"hn_preprocess_bgr {name}")
    want = R.preprocess(frames, (hd, wd))
    got = dst.view.cpu().numpy().reshape(n, 3, hd, wd)
    bad = np.argwhere(got.view(np.int32) != want.view(np.int32))
    assert not len(bad), (f"hn_preprocess_bgr {name}: {len(bad)} of {got.size} values differ, first (n, c, y, x) {bad[:6].tolist()}: got "
                          f"{got[tuple(bad[0])]!r} want {want[tuple(bad[0])]!r}")


# =====================================================================================================================================
# seg confusion counts
# =====================================================================================================================================
@pytest.mark.parametrize("C", Cs.CONF_C)
def test_seg_confusion(L, C):
    """int64 then float32 targets into ONE matrix per M (the second call accumulates); ids 255, C, C + 1, 2^40, float 4.99 / 255.0, and
    negative ids on both sides, which count in the ignore bucket C"""
    nb = (C + 1) ** 2
    for M in Cs.CONF_M:
        conf = GuardedBytes(nb * 8, fill=0)
        total = np.zeros((C + 1, C + 1), np.int64)
        for is_float in (False, True):
            pred, target = Cs.confusion_case(C, M, is_float)
            assert (pred < 0).any() and (M == 1 or (target < 0).any())
            p, t = D(pred), D(target)
            assert rc_of(L, "hn_seg_confusion", p.data_ptr(), t.data_ptr(), int(is_float), M, C, conf.ptr()) == 0
            torch.cuda.synchronize()
            total += R.confusion(pred, target, C)
            got = conf.as_(torch.int64, C + 1, C + 1).cpu().numpy()
            conf.check(f"hn_seg_confusion C={C} M={M}")
            bad = np.argwhere(got != total)
            assert not len(bad), (f"hn_seg_confusion C={C} M={M} after the {'float32' if is_float else 'int64'} call: (pred, target) buckets "
                                  f"{bad[:6].tolist()} hold {[int(got[tuple(b)]) for b in bad[:6]]}, want {[int(total[tuple(b)]) for b in bad[:6]]}")
        assert int(total.sum()) == 2 * M


def test_seg_confusion_negative_ids_go_to_the_ignore_bucket(L):
    """the reference raises on a negative id; counting it as class 0 (what the kernel did) inflates class 0's false positives / negatives"""
    pred = np.array([-1, 0, 0, -(1 << 40), 2, -5], np.int64)
    tgt = np.array([0, -1, 0, -3, -(1 << 40), 1], np.int64)
    tgf = np.array([0.0, -1.0, 0.0, -3.5, -1e12, 1.0], np.float32)
    want = np.zeros((4, 4), np.int64)
    for p, t in ((3, 0), (0, 3), (0, 0), (3, 3), (2, 3), (3, 1)):
        want[p, t] += 1
    assert np.array_equal(R.confusion(pred, tgt, 3), want) and np.array_equal(R.confusion(pred, tgf, 3), want)
    for is_float, t in ((0, tgt), (1, tgf)):
        conf = GuardedBytes(16 * 8, fill=0)
        p_d, t_d = D(pred), D(t)
        assert rc_of(L, "hn_seg_confusion", p_d.data_ptr(), t_d.data_ptr(), is_float, 6, 3, conf.ptr()) == 0
        torch.cuda.synchronize()
        conf.check("hn_seg_confusion negative ids")
        got = conf.as_(torch.int64, 4, 4).cpu().numpy()
        assert np.array_equal(got, want), f"negative ids (float target: {bool(is_float)}): got\n{got}\nwant\n{want}"
        assert got[0].sum() + got[:, 0].sum() - got[0, 0] == 3                              # class 0 sees only its own three pixels


def test_seg_confusion_refuses_64_classes(L):
    conf = GuardedBytes(65 * 65 * 8)
    p = D(np.zeros(16, np.int64))
    assert rc_of(L, "hn_seg_confusion", p.data_ptr(), p.data_ptr(), 0, 16, 64, conf.ptr()) == HN_ERR_ARG
    torch.cuda.synchronize()
    conf.check("hn_seg_confusion C=64")
    assert conf.untouched()


# =====================================================================================================================================
# seg overlay
# =====================================================================================================================================
@pytest.mark.parametrize("case", Cs.OVERLAY_SHAPES, ids=[c[0] for c in Cs.OVERLAY_SHAPES])
def test_seg_overlay(L, case):
    name, n, (h, w), (ho, wo) = case
    mask, frames = Cs.overlay_case(*case)
    m, lut, f = D(mask), D(Cs.LUT), D(frames)
    out = GuardedBytes(n * ho * wo * 3)
    assert rc_of(L, "hn_seg_overlay", m.data_ptr(), n, h, w, lut.data_ptr(), len(Cs.LUT), f.data_ptr(), out.ptr(), ho, wo) == 0
    torch.cuda.synchronize()
    out.check(f"hn_seg_overlay {name}")
    want = R.overlay(mask, Cs.LUT, frames)
    got = out.as_(torch.uint8, n, ho, wo, 3).cpu().numpy()
    bad = np.argwhere(got != want)
    assert not len(bad), (f"hn_seg_overlay {name}: {len(bad)} of {got.size} bytes differ, first (n, y, x, c) {bad[:6].tolist()}: got "
                          f"{[int(got[tuple(b)]) for b in bad[:6]]} want {[int(want[tuple(b)]) for b in bad[:6]]}")
    if name == "identity":
        assert got[0, 0].tolist() == [[0, 2, 2]] * wo and got[0, 1].tolist() == [[255, 255, 255]] * wo


# =====================================================================================================================================
# lane rasteriser and pair counts
# =====================================================================================================================================
def raster_on_device(L, lanes, lw, H, W):
    pts, seg_lane, seg_first = Cs.pack_segments(lanes)
    masks = GuardedBytes(len(lanes) * H * W, fill=0)
    tp, tl, tf = D(pts), D(seg_lane), D(seg_first)
    assert rc_of(L, "hn_lane_raster", tp.data_ptr(), tl.data_ptr(), tf.data_ptr(), len(seg_lane), lw, H, W, masks.ptr()) == 0
    torch.cuda.synchronize()
    masks.check(f"hn_lane_raster width {lw}")
    return masks.as_(torch.uint8, len(lanes), H, W), R.raster(pts, seg_lane, seg_first, lw, H, W, n_lanes=len(lanes))


@pytest.mark.parametrize("lw", Cs.LANE_WIDTHS)
def test_lane_raster(L, lw):
    H, W = Cs.RASTER_HW
    got, want = raster_on_device(L, Cs.raster_lanes(), lw, H, W)
    got = got.cpu().numpy()
    bad = np.argwhere(got != want)
    assert not len(bad), (f"hn_lane_raster width {lw}: {len(bad)} pixels differ, first (lane, y, x) {bad[:8].tolist()}: got "
                          f"{[int(got[tuple(b)]) for b in bad[:8]]} want {[int(want[tuple(b)]) for b in bad[:8]]}")
    assert want[1].sum() > 0 and want[8].sum() == 0 and want[9].sum() == 0                  # the zero-length disc; the unreachable lanes


@pytest.mark.parametrize("G,P", Cs.PAIR_SHAPES)
def test_lane_iou_counts(L, G, P):
    """the device's own masks of G + P lanes, padded to HW = 24 * 40 + 1 (not a multiple of 256) with one more pixel set in the last
    ground truth and the last prediction (lane 31 = bit 31 of the per-pixel words at 32 lanes)"""
    H, W = Cs.RASTER_HW
    gts, prs = Cs.pair_lanes(G, P)
    got, want = raster_on_device(L, gts + prs, 3, H, W)
    assert torch.equal(got.cpu(), torch.from_numpy(want)) and all(want[j].any() for j in range(G + P))
    HW = H * W + 1
    padded = torch.zeros((G + P, HW), dtype=torch.uint8, device=dev())
    padded[:, :H * W] = got.reshape(G + P, -1)
    padded[G - 1, -1] = padded[G + P - 1, -1] = 255
    inter, area = GuardedBytes(G * P * 8, fill=0), GuardedBytes((G + P) * 8, fill=0)
    assert rc_of(L, "hn_lane_iou", padded.data_ptr(), G, P, HW, inter.ptr(), area.ptr()) == 0
    torch.cuda.synchronize()
    inter.check(f"hn_lane_iou {G}x{P} inter")
    area.check(f"hn_lane_iou {G}x{P} area")
    wi, wa = R.pair_counts(padded.cpu().numpy(), G, P)
    gi, ga = inter.as_(torch.int64, G, P).cpu().numpy(), area.as_(torch.int64, G + P).cpu().numpy()
    assert np.array_equal(ga, wa), f"hn_lane_iou {G}x{P}: areas differ at lanes {np.argwhere(ga != wa)[:6, 0].tolist()}: got {ga.tolist()} want {wa.tolist()}"
    bad = np.argwhere(gi != wi)
    assert not len(bad), f"hn_lane_iou {G}x{P}: |g & p| differs at (g, p) {bad[:6].tolist()}: got {[int(gi[tuple(b)]) for b in bad[:6]]} want {[int(wi[tuple(b)]) for b in bad[:6]]}"
    assert wi[G - 1, P - 1] > 0 and wa[G - 1] > 0 and wa[G + P - 1] > 0
