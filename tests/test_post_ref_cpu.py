"""Holds tests/post_ref.py (the references of tests/test_post_exact_gpu.py) to the oracle's own loop-form functions on the cases of
tests/post_cases.py, exactly, without a GPU; shows for every mutant of a reference a GPU case whose expected output it changes (the
suite would notice a kernel with that fault; no wrong kernel is ever run); and asserts the caps the lane cases state: at most 200
candidates per image above 1024 anchors, probabilities tied or 1e-3 apart, on the threshold or 1e-3 from it."""
import numpy as np
import pytest
import torch

from oracle import hydranet_oracle as O
from tests import post_cases as Cs
from tests import post_ref as R

F32 = np.float32


def lane_cases():
    out = dict(("content/" + k, v) for k, v in Cs.lane_content_cases().items())
    for g in Cs.GEOMETRIES:
        out["geometry/" + g[0]] = Cs.lane_geometry_case(*g)
    return out


LANE = lane_cases()


def lane_ref(c, mutant=None):
    return R.lane_decode_nms(c["cls"], c["loc"], c["geometry"], c["thr"], c["nms_thr"], c["use_mean"], c["margin"], mutant=mutant)


def lane_flat(r):
    """the expected raw outputs as a list of arrays (NaN = unwritten X)"""
    return [r["prob"], r["start"], r["end"], np.nan_to_num(r["X"], nan=-12345.0), r["written"], r["count"], np.concatenate(r["order"]),
            np.concatenate(r["keep"])]


def same(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a, b))


# =====================================================================================================================================
# the restatements against the oracle
# =====================================================================================================================================
@pytest.mark.parametrize("name", list(LANE))
def test_lane_decode_nms_equals_the_oracle(name):
    c = LANE[name]
    r = lane_ref(c)
    W, H, stride, ppl = c["geometry"]
    geo = O.LaneGeometry(W, H, stride, ppl)
    for n in range(c["cls"].shape[0]):
        lanes = O.lane_decode(geo, c["cls"][n], c["loc"][n], c["thr"], c["margin"])
        valid = np.nonzero(r["end"][n] - r["start"][n] >= 2)[0]
        assert [l["anchor"] for l in lanes] == valid.tolist()
        for l in lanes:
            a = l["anchor"]
            s, e = int(r["start"][n, a]), int(r["end"][n, a])
            assert (l["start_pos"], l["end_pos"]) == (s, e)
            assert l["prob"] == float(r["prob"][n, a])
            assert np.array_equal(l["xs"], r["X"][n, a, s:e]) and l["xs"].dtype == F32
        assert [l["anchor"] for l in O.lane_nms(lanes, -1.0, bool(c["use_mean"]))] == r["order"][n].tolist()
        kept = O.lane_nms(lanes, c["nms_thr"], bool(c["use_mean"]))
        assert [l["anchor"] for l in kept] == r["order"][n][r["keep"][n] == 1].tolist()
        assert r["count"][n] == len(lanes)


def test_lane_content_cases_hold_what_they_claim():
    cs = Cs.lane_content_cases()
    r = lane_ref(cs["margin100"])
    assert r["count"].tolist()[1:] == [0, 32] and r["count"][0] > 8                       # an empty image and a full one in the batch
    st, en = r["start"][0], r["end"][0]
    o, k = r["order"][0].tolist(), r["keep"][0]
    alive = {a: int(k[o.index(a)]) for a in o}
    assert (alive[24], alive[25], alive[26]) == (1, 0, 1)                                  # A kills B at dis == thr; B is dead, so C lives
    assert (st[27], en[27]) == (0, 1) and 27 not in o and r["written"][0, 27].sum() == 1   # one point: written, no lane
    assert (st[28], en[28]) == (0, 2) and 28 in o                                          # two points, prob == thr: a lane
    assert r["prob"][0, 28] == F32(0.5) and (st[29], en[29]) == (0, 1)
    assert (st[30], en[30]) == (0, 3)                                                      # the up walk stops at ax == W
    assert (st[16], en[16]) == (3, 7) and (st[17], en[17]) == (1, 4) and (st[18], en[18]) == (0, 4) and (st[19], en[19]) == (4, 16)
    assert (st[22], en[22]) == (2, 6) and r["X"][0, 22, 5] == 0.0                          # ax == 0 is kept, ax == -8 stops the walk
    assert (st[23], en[23]) == (1, 6) and r["X"][0, 23, 1] == 352.0                        # W <= ax < W + margin on the down walk
    assert (st[0], en[0]) == (0, 16) and (st[4], en[4]) == (12, 16)
    r0 = lane_ref(cs["margin0"])
    assert (r0["start"][0, 23], r0["end"][0, 23]) == (3, 6)                                # margin 0: the down walk stops at ax == W too
    rn = lane_ref(cs["thr_next"])
    assert 28 not in rn["order"][0].tolist() and (rn["start"][0, 28], rn["end"][0, 28]) == (0, 0) and rn["count"][0] == r["count"][0] - 3
    # ties: anchors of one probability appear in raster order, groups interleaved in raster order
    p0 = r["prob"][0]
    for group in ([8, 10, 12, 26], [9, 11, 14, 25], [13, 15, 28]):
        assert len(set(p0[group].tolist())) == 1 and [a for a in o if a in group] == group
    rm = lane_ref(cs["use_mean"])
    om = rm["order"][0].tolist()
    assert alive[21] == 1 and rm["keep"][0][om.index(21)] == 0                             # mean 12 <= 24 < maximum 48
    assert all(int(x.all()) for x in lane_ref(cs["nms_off"])["keep"])
    rw = lane_ref(cs["nms_wide"])
    ow = rw["order"][0].tolist()
    assert rw["keep"][0][ow.index(4)] == 1 or rw["keep"][0][ow.index(28)] == 1             # (pairs without overlap never suppress)
    assert 1 < int(rw["keep"][0].sum()) < r["keep"][0].sum()


def test_lane_case_caps():
    for name, c in LANE.items():
        r = lane_ref(c)
        hw = c["cls"].shape[1]
        assert R.lane_geometry(*c["geometry"])["hw"] == hw <= 7168
        if hw > 1024:
            cand = (~(r["prob"] < F32(c["thr"]))).sum(1)
            assert int(cand.max()) <= 200 and int(r["count"].max()) <= 200, name
            assert int(r["count"].min()) >= len(c["planted"]) >= 3
        thr = F32(c["thr"])
        for n in range(r["prob"].shape[0]):
            p = np.unique(r["prob"][n].astype(np.float64))
            assert len(p) == 1 or float(np.diff(p).min()) >= 1e-3, (name, n)
            # on the threshold, or 1e-3 from it.  The one exception is the `thr_next` case, whose threshold is one place above 0.5:
            # the probability of EQUAL logits is exp(0) / (exp(0) + exp(0)) = 1 / 2 in every softmax form, device expf included, so the
            # value 0.5 itself carries no last-place doubt and may sit next to the threshold
            equal_logits = c["cls"][n, :, 0] == c["cls"][n, :, 1]
            assert bool((r["prob"][n][equal_logits] == F32(0.5)).all())
            d = np.abs(p - float(thr))
            assert bool(((d == 0) | (d >= 1e-3) | (p == 0.5)).all()), (name, n)
            assert bool((r["prob"][n][~equal_logits] != F32(0.5)).all())
    lds = {g[0]: R.lane_lds_bytes(g[1] * g[2]) for g in Cs.GEOMETRIES}
    assert lds["60x51"] <= 65536 < lds["60x52"] and Cs.GEOMETRIES[3][1] * Cs.GEOMETRIES[3][2] == 7168
    assert Cs.REFUSED_GEOMETRY[1] * Cs.REFUSED_GEOMETRY[2] == 7232
    g18 = R.lane_geometry(*LANE["geometry/8x4_ppl18"]["geometry"])
    assert g18["ppa"] == 4.5 and float(g18["interval"]) != round(float(g18["interval"]))
    for name in ("35x32", "60x51", "60x52", "112x64"):
        c = LANE["geometry/" + name]
        hw = c["cls"].shape[1]
        assert c["planted"] == sorted({a for a in (0, 1023, 1024, 2047, 2048, hw - 1) if a < hw})
        r = lane_ref(c)
        for n in range(2):
            assert set(c["planted"]) <= set(r["order"][n].tolist())


@pytest.mark.parametrize("case", Cs.PREPROCESS_SHAPES, ids=[c[0] for c in Cs.PREPROCESS_SHAPES])
def test_preprocess_equals_the_oracle(case):
    name, n, shw, dhw = case
    frames = Cs.preprocess_case(*case)
    assert frames.min() == 0 and frames.max() == 255
    got = R.preprocess(frames, dhw)
    assert got.dtype == F32 and got.shape == (n, 3) + dhw
    for i in range(n):
        assert np.array_equal(got[i], O.preprocess_bgr(frames[i], dhw))


def conf_stats(conf, C):
    tp = np.diagonal(conf)[:C]
    return tp, conf.sum(1)[:C] - tp, conf.sum(0)[:C] - tp, conf.sum(0)[:C]


@pytest.mark.parametrize("is_float", [False, True], ids=["int64", "float32"])
@pytest.mark.parametrize("C", Cs.CONF_C)
def test_confusion_equals_the_oracle(C, is_float):
    for M in Cs.CONF_M:
        pred, target = Cs.confusion_case(C, M, is_float, negatives=False)
        conf = R.confusion(pred, target, C)
        assert conf.dtype == np.int64 and conf.shape == (C + 1, C + 1) and int(conf.sum()) == M
        ref = O.seg_stat_scores(torch.from_numpy(pred), torch.from_numpy(target), C)
        for a, b in zip(conf_stats(conf, C), ref):
            assert np.array_equal(a, b.numpy())
        pn, tn = Cs.confusion_case(C, M, is_float)
        assert (pn < 0).any() and (M == 1 or (tn < 0).any())
        with pytest.raises((RuntimeError, IndexError)):                                   # the reference has no value for a negative id
            O.seg_stat_scores(torch.from_numpy(pn), torch.from_numpy(tn), C)
    p = np.array([0, -1, 0, 3, -7], np.int64)
    t = np.array([-1, 0, 0, -(1 << 40), -2], np.int64)
    want = np.zeros((2, 2), np.int64)
    want[0, 1], want[1, 0], want[0, 0], want[1, 1] = 1, 1, 1, 2
    assert np.array_equal(R.confusion(p, t, 1), want)
    assert np.array_equal(R.confusion(np.zeros(4, np.int64), np.array([4.99, 0.99, -0.5, 5.0], F32), 5)[0], [2, 0, 0, 0, 1, 1])


def lut_dict():
    return {i: tuple(int(v) for v in Cs.LUT[i]) for i in range(len(Cs.LUT))}


@pytest.mark.parametrize("case", Cs.OVERLAY_SHAPES, ids=[c[0] for c in Cs.OVERLAY_SHAPES])
def test_overlay_equals_the_oracle(case):
    name, n, mhw, fhw = case
    mask, frames = Cs.overlay_case(*case)
    got = R.overlay(mask, Cs.LUT, frames)
    ref = O.seg_decode(list(frames), torch.from_numpy(mask), (fhw[1], fhw[0]), lut_dict())
    assert got.dtype == np.uint8 and np.array_equal(got, np.stack(ref))
    assert {-1, 5, 1 << 33} <= set(mask.reshape(-1).tolist()) or mask.size < 8
    if name == "identity":
        assert got[0, 0].tolist() == [[0, 2, 2]] * fhw[1]                                  # 0.5, 1.5, 2.5: half to even
        assert got[0, 1].tolist() == [[255, 255, 255]] * fhw[1]                            # 204 + 127.5 saturates
        assert got[1, 2, :3].tolist() == [[160, 160, 160]] * 3                             # out-of-range ids: black, 0.8 * 200


def test_raster_equals_the_oracle():
    H, W = Cs.RASTER_HW
    lanes = Cs.raster_lanes()
    pts, seg_lane, seg_first = Cs.pack_segments(lanes)
    for lw in Cs.LANE_WIDTHS:
        got = R.raster(pts, seg_lane, seg_first, lw, H, W, n_lanes=len(lanes))
        for j, lane in enumerate(lanes):
            im = np.zeros((H, W), np.uint8)
            for p0, p1 in zip(lane[:-1], lane[1:]):
                O.cv2_line(im, p0, p1, 255, lw)
            assert np.array_equal(got[j], im), (lw, j)
        assert got[8].sum() == 0 and got[9].sum() == 0                                     # out of reach: empty bounding boxes
        assert (got[6].sum() > 0) == (lw >= 30) and got[1].sum() > 0 and all(got[j].sum() > 0 for j in (2, 3, 4, 5, 10, 11))
    assert R.raster(pts, seg_lane, seg_first, 1, H, W, n_lanes=len(lanes))[1].sum() == 255  # the zero-length segment at width 1: one pixel


def pair_case(G, P, lw=3):
    """masks [G + P, 24 * 40 + 1]: the rasterised lanes, padded by one pixel that ground truth G - 1 and prediction P - 1 set"""
    H, W = Cs.RASTER_HW
    gts, prs = Cs.pair_lanes(G, P)
    pts, seg_lane, seg_first = Cs.pack_segments(gts + prs)
    m = R.raster(pts, seg_lane, seg_first, lw, H, W, n_lanes=G + P)
    padded = np.zeros((G + P, H * W + 1), np.uint8)
    padded[:, :H * W] = m.reshape(G + P, -1)
    padded[G - 1, -1] = padded[G + P - 1, -1] = 255
    return gts, prs, m, padded


@pytest.mark.parametrize("G,P", Cs.PAIR_SHAPES)
def test_pair_counts_equal_the_oracle(G, P):
    H, W = Cs.RASTER_HW
    gts, prs, m, padded = pair_case(G, P)
    inter, area = R.pair_counts(m.reshape(G + P, -1), G, P)
    assert int(area.min()) > 0 and int(inter.max()) > 0
    for g in range(0, G, 5):
        for p in range(0, P, 3):
            # the oracle rasterises the unit-step samples of the spline through the points, truncated: the same samples through raster()
            ims = []
            for lane in (gts[g], prs[p]):
                ip = O.lane_spline_interp([{"x": float(x), "y": float(y)} for x, y in lane], 1)
                q = [(int(s["x"]), int(s["y"])) for s in ip]
                ps, sl, sf = Cs.pack_segments([q])
                ims.append(R.raster(ps, sl, sf, 3, H, W, n_lanes=1)[0])
            i2, a2 = R.pair_counts(np.stack(ims).reshape(2, -1), 1, 1)
            union = a2[0] + a2[1] - i2[0, 0]
            want = O.lane_iou([{"x": float(x), "y": float(y)} for x, y in gts[g]], [{"x": float(x), "y": float(y)} for x, y in prs[p]], H, W, 3)
            assert (0 if union == 0 else i2[0, 0] / union) == want
    ip, ap = R.pair_counts(padded, G, P)
    assert ip[G - 1, P - 1] == inter[G - 1, P - 1] + 1 and ap[G - 1] == area[G - 1] + 1 and ap[G + P - 1] == area[G + P - 1] + 1
    brute = np.array([[int(((padded[g] != 0) & (padded[G + p] != 0)).sum()) for p in range(P)] for g in range(G)])
    assert np.array_equal(ip, brute) and np.array_equal(ap, (padded != 0).sum(1))


# =====================================================================================================================================
# every mutant of a reference changes the expected output of at least one GPU case
# =====================================================================================================================================
def expected_outputs(fn, mutant):
    """name -> expected output(s) of every GPU case of one entry point under `mutant` (None: the reference itself); an out-of-range read of
    the mutant (IndexError) is an output of its own"""
    out = {}
    if fn == "lane_decode_nms":
        for name, c in LANE.items():
            out[name] = lane_flat(lane_ref(c, mutant))
    elif fn == "confusion":
        for C in Cs.CONF_C:
            for M in Cs.CONF_M:
                for fl in (False, True):
                    out[f"C{C}_M{M}_{'f32' if fl else 'i64'}"] = [R.confusion(*Cs.confusion_case(C, M, fl), C, mutant=mutant)]
    elif fn in ("overlay", "preprocess"):
        for case in (Cs.OVERLAY_SHAPES if fn == "overlay" else Cs.PREPROCESS_SHAPES):
            try:
                if fn == "overlay":
                    mask, frames = Cs.overlay_case(*case)
                    out[case[0]] = [R.overlay(mask, Cs.LUT, frames, mutant=mutant)]
                else:
                    out[case[0]] = [R.preprocess(Cs.preprocess_case(*case), case[3], mutant=mutant)]
            except IndexError:
                out[case[0]] = [np.array(["reads outside the source"])]
    elif fn == "raster":
        H, W = Cs.RASTER_HW
        lanes = Cs.raster_lanes()
        pts, seg_lane, seg_first = Cs.pack_segments(lanes)
        for lw in Cs.LANE_WIDTHS:
            out[f"width{lw}"] = [R.raster(pts, seg_lane, seg_first, lw, H, W, n_lanes=len(lanes), mutant=mutant)]
    elif fn == "pair_counts":
        for G, P in Cs.PAIR_SHAPES:
            out[f"{G}x{P}"] = list(R.pair_counts(pair_case(G, P)[3], G, P, mutant=mutant))
    return out


CAUGHT_BY = {}


@pytest.mark.parametrize("fn,mutant", [(fn, m) for fn, ms in R.MUTANTS.items() for m in ms])
def test_every_mutant_changes_an_expected_output(fn, mutant):
    ref, mut = expected_outputs(fn, None), expected_outputs(fn, mutant)
    caught = [name for name in ref if not same(ref[name], mut[name])]
    CAUGHT_BY[(fn, mutant)] = caught
    print(f"{fn} mutant {mutant}: caught by {caught}")
    assert caught, f"no GPU case of {fn} has an expected output that the mutant {mutant} changes"
