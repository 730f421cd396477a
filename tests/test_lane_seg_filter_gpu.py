"""GPU: the lane filter by the seg head's marking class (hn_lane_filter.hip, lane_codec.LaneSegFilter, Demo(lane_seg_filter=))
against its numpy restatement (tests/lane_seg_filter_ref.py).  Every check compares integers or lists for equality: no tolerance anywhere.
Kernel level: synthetic decode arrays straight into hn_lane_seg_filter; decode_batch level: synthetic logits; demo level: the tiny cfg with
its recorded weights on two synthetic frames."""
import numpy as np
import pytest
import torch

from tests import lane_seg_filter_ref as R
from tests.helpers import load_cfg, load_npz, tiny_state

pytestmark = pytest.mark.gpu

SHAPES = {"96x160": (96, 160), "128x128": (128, 128)}                   # (H, W); stride 32, interval 8: 15 anchors of 12 points, 16 of 16
STRIDE, INTERVAL = 32, 8
ZIGZAG, DIAGONAL = 5, 0                                                 # anchors of the lanes some checks speak of


def decode_arrays(H, W):
    """hn_lane_decode_nms's outputs, made by hand for N = 3 images: counts 0 (its rows hold garbage that must not be read), 1, and every
    anchor.  X is NaN wherever no point lives."""
    hw, ppl = (H // STRIDE) * (W // STRIDE), H // INTERVAL
    g = np.random.Generator(np.random.Philox(5))
    X = np.full((3, hw, ppl), np.nan, np.float32)
    start, end = np.zeros((3, hw), np.int32), np.zeros((3, hw), np.int32)
    p = np.arange(ppl, dtype=np.float32)

    def lane(n, a, s, e, xs):
        start[n, a], end[n, a] = s, e
        X[n, a, s:e] = np.asarray(xs, np.float32)[s:e]

    lane(2, 0, 0, ppl, 40 + 6 * p)                                      # crosses x = 64 and y = 64
    lane(2, 1, 0, ppl, W - 20 + 10 * p)                                 # runs out of the image on the right (the down-branch margin)
    lane(2, 2, 1, ppl - 1, 20.5 + p)                                    # ties: 20.5 -> 20, 21.5 -> 22, 22.5 -> 22, ...
    lane(2, 3, 0, ppl, 30 + 2 * p)
    X[2, 3, 4] = np.nan                                                 # a NaN inside the range: paints nothing
    lane(2, 4, 3, 4, 50 + p)                                            # a single point
    lane(2, ZIGZAG, 0, ppl, np.where(np.arange(ppl) % 2 == 0, 70, 76))  # segments that overlap each other
    lane(2, 6, 0, ppl, 90 + p)                                          # (its keep entry is 0)
    lane(2, 7, 2, ppl, np.full(ppl, 64))                                # on the tile border
    lane(2, 8, 2, 9, 10 + 3 * p)                                        # NaN outside its range only
    lane(2, 9, 0, ppl, -30 + 4 * p)                                     # partly left of the image
    lane(2, 10, 0, 5, np.full(ppl, 1e9))                                # clamped to 16383: nothing inside the image
    lane(2, 11, 0, ppl, np.where(np.arange(ppl) == 3, np.inf, 100.0))   # an infinity
    for a in range(12, hw):
        lane(2, a, int(g.integers(0, 3)), int(g.integers(ppl - 4, ppl + 1)), np.cumsum(g.normal(0, 5, ppl)) + g.integers(10, W - 10))
    lane(1, 4, 0, ppl, 70 - 3 * p + 0.25)
    lane(0, 2, 0, ppl, 20 + p)                                          # image 0 has lanes, but counts[0] = 0
    order = np.zeros((3, hw), np.int32)
    keep = np.zeros((3, hw), np.int32)
    order[2] = [6, DIAGONAL, ZIGZAG] + [a for a in range(hw) if a not in (6, DIAGONAL, ZIGZAG)]
    keep[2] = 1
    keep[2, 0] = 0                                                      # the first candidate was suppressed: the selection skips it
    order[1, 0], keep[1, 0] = 4, 1
    order[1, 1:], keep[1, 1:] = 3, 1                                    # beyond counts[1]: not candidates
    order[0], keep[0] = 2, 1
    counts = np.array([0, 1, hw], np.int32)
    if hw == 16:
        assert int(keep[2].sum()) > 14                                  # the cap of 14 cuts
    return dict(X=X, start=start, end=end, order=order, keep=keep, counts=counts, hw=hw, ppl=ppl, H=H, W=W)


def class_map(kind, H, W):
    g = np.random.Generator(np.random.Philox(9))
    if kind == "random":
        return g.integers(0, 5, (3, H, W)).astype(np.int64)
    if kind == "none":
        return g.choice(np.array([0, 1, 3, 4]), (3, H, W)).astype(np.int64)
    return np.full((3, H, W), 2, np.int64)


def run_kernel(A, mask, lane_class=2, line_width=20, min_ratio=0.01, top_k=14):
    """hn_lane_seg_filter twice, each time into buffers of 0x7f bytes -> (keep_out, stats, n_sel) of the first run, equal to the second's"""
    from multitask_hydranet_amd._lib import lib
    dev = torch.device("cuda:0")
    d = {k: torch.from_numpy(A[k]).to(dev) for k in ("X", "start", "end", "order", "keep", "counts")}
    m = torch.from_numpy(mask).to(dev)
    N, hw, ppl = 3, A["hw"], A["ppl"]
    need = lib().query("hn_lane_seg_filter_ws_bytes", N, top_k, ppl)
    assert need > 0
    runs = []
    for _ in range(2):
        ws = torch.full((need,), 0x7f, device=dev, dtype=torch.uint8)
        keep_out = torch.full((N, hw), 0x7f7f7f7f, device=dev, dtype=torch.int32)
        stats = torch.full((N, top_k, 4), 0x7f7f7f7f, device=dev, dtype=torch.int32)
        n_sel = torch.full((N,), 0x7f7f7f7f, device=dev, dtype=torch.int32)
        lib().call("hn_lane_seg_filter", d["X"].data_ptr(), d["start"].data_ptr(), d["end"].data_ptr(), d["order"].data_ptr(), d["keep"].data_ptr(),
                   d["counts"].data_ptr(), N, A["W"], A["H"], STRIDE, ppl, INTERVAL, m.data_ptr(), lane_class, line_width, float(min_ratio), top_k,
                   ws.data_ptr(), need, keep_out.data_ptr(), stats.data_ptr(), n_sel.data_ptr())
        runs.append((keep_out.cpu().numpy(), stats.cpu().numpy(), n_sel.cpu().numpy()))
    for a, b in zip(*runs):
        assert np.array_equal(a, b)
    for k in ("X", "start", "end", "order", "keep", "counts"):
        assert np.array_equal(d[k].cpu().numpy(), A[k], equal_nan=True)  # the inputs are untouched
    return runs[0]


def reference(A, mask, lane_class=2, line_width=20, min_ratio=0.01, top_k=14):
    return R.seg_filter(A["X"], A["start"], A["end"], A["order"], A["keep"], A["counts"], A["W"], A["H"], STRIDE, A["ppl"], INTERVAL, mask,
                        lane_class, line_width, min_ratio, top_k)


def assert_same(got, want):
    for name, a, b in zip(("keep_out", "stats", "n_sel"), got, want):
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), (name, a.tolist(), b.tolist())


@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("top_k", [2, 14])
@pytest.mark.parametrize("kind", ["random", "none", "all"])
def test_kernel_equals_the_reference(shape, top_k, kind):
    H, W = SHAPES[shape]
    A = decode_arrays(H, W)
    mask = class_map(kind, H, W)
    want = reference(A, mask, top_k=top_k)
    got = run_kernel(A, mask, top_k=top_k)
    assert_same(got, want)
    keep_out, stats, n_sel = got
    assert n_sel.tolist() == [0, 1, min(top_k, int(A["keep"][2].sum()))]
    assert stats[2, 0, 0] == 1 and stats[2, 1, 0] == 2                   # the suppressed first candidate was skipped
    assert stats[2, :, 1].max() > 0 and stats[1, 0, 1] > 0
    if kind == "none":
        assert not stats[:, :, 3].any() and not keep_out.any()
    if kind == "all":
        assert np.array_equal(stats[:, :, 3], (stats[:, :, 1] > 0).astype(np.int32)) and np.array_equal(stats[:, :, 2], stats[:, :, 1])
    if top_k == 14:                                                      # the lanes that paint nothing were selected, and dropped
        by_anchor = {int(A["order"][2, j]): (area, kept) for j, area, _, kept in stats[2, :n_sel[2]].tolist()}
        for a in (3, 4, 10, 11):
            assert by_anchor[a] == (0, 0), a
        assert by_anchor[1][0] > 0 and by_anchor[9][0] > 0               # clipped on the right and on the left, not lost


def test_the_cases_are_not_vacuous():
    for H, W in SHAPES.values():
        A = decode_arrays(H, W)
        pts = R.lane_points(A["X"][2, ZIGZAG], 0, A["ppl"], H, INTERVAL)
        union = int(R.lane_mask(pts, H, W, 20).sum())
        per_segment = sum(int(R.lane_mask([a, b], H, W, 20).sum()) for a, b in zip(pts, pts[1:]))
        assert 0 < union < per_segment                                   # overlapping segments: a pixel counts once
        xs = [x for x, _ in R.lane_points(A["X"][2, 2], 1, A["ppl"] - 1, H, INTERVAL)]
        assert xs[:4] == [22, 22, 24, 24]                                # 21.5, 22.5, 23.5, 24.5: ties went to even
        d = R.lane_points(A["X"][2, DIAGONAL], 0, A["ppl"], H, INTERVAL)
        assert min(x for x, _ in d) < 64 < max(x for x, _ in d) and min(y for _, y in d) < 64 < max(y for _, y in d)
        assert max(x for x, _ in R.lane_points(A["X"][2, 1], 0, A["ppl"], H, INTERVAL)) > W + 20
        assert H % 64 or W % 64 or (H, W) == (128, 128)                  # 96 x 160: tiles that end outside the image in both directions


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_the_decision_is_strict_at_the_exact_ratio(shape):
    H, W = SHAPES[shape]
    A = decode_arrays(H, W)
    mask = class_map("random", H, W)
    _, stats, n_sel = reference(A, mask)
    k = next(k for k in range(n_sel[2]) if 0 < stats[2, k, 2] < stats[2, k, 1])
    ratio = np.float32(stats[2, k, 2]) / np.float32(stats[2, k, 1])
    below = np.nextafter(ratio, np.float32(-1))
    assert below < ratio
    for thr, kept in ((ratio, 0), (below, 1)):
        want = reference(A, mask, min_ratio=float(thr))
        got = run_kernel(A, mask, min_ratio=float(thr))
        assert_same(got, want)
        assert got[1][2, k, 3] == kept and got[0][2, stats[2, k, 0]] == kept


def test_other_class_width_and_a_single_lane_cap():
    A = decode_arrays(96, 160)
    mask = class_map("random", 96, 160)
    for kw in (dict(lane_class=4, line_width=1, top_k=1), dict(lane_class=0, line_width=7, min_ratio=0.25, top_k=64),
               dict(lane_class=3, line_width=64, min_ratio=0.2, top_k=5)):
        assert_same(run_kernel(A, mask, **kw), reference(A, mask, **kw))


# ---- decode_batch ----------------------------------------------------------------------------------------------------------------------
def lane_key(ln):
    return (float(ln.prob), int(ln.start_pos), int(ln.end_pos), float(ln.ax), float(ln.ay), [(float(p.x), float(p.y)) for p in ln.lane])


@pytest.fixture(scope="module")
def synthetic_head():
    """logits of N = 2 images at 128 x 128 (16 anchors of 16 points): the four bottom-row anchors carry lanes that lean to the right, 32
    pixels apart; class 2 fills the left half of image 0 and the right half of image 1"""
    from multitask_hydranet_amd.lane_codec import LaneCodec
    codec = LaneCodec(128, 128, 32, 16)
    cls = np.zeros((2, 16, 2), np.float32)
    cls[:, :, 0] = 4.0
    loc = np.zeros((2, 16, 34), np.float32)
    for n in range(2):
        for w in range(4):
            a = 12 + w
            cls[n, a] = (0.0, 3.0 + 0.5 * ((w + n) % 4))
            loc[n, a, 17] = 10 + w                                       # points upward from the anchor's row
            loc[n, a, 18:34] = 0.05 * (1 + n) * np.arange(16)
    mask = np.zeros((2, 128, 128), np.int64)
    mask[0, :, :64] = 2
    mask[1, :, 64:] = 2
    mask[:, ::3, :] += 1                                                 # stripes of other classes (1 and 3)
    dev = torch.device("cuda:0")
    return codec, torch.from_numpy(cls).to(dev), torch.from_numpy(loc).to(dev), mask


def test_decode_batch_with_the_filter_off_is_unchanged(synthetic_head):
    from multitask_hydranet_amd import lane_codec as LC
    from multitask_hydranet_amd._lib import lib
    codec, cls, loc, mask = synthetic_head
    plain = LC.decode_batch(cls, loc, codec, 0.5, 10, False)
    off = LC.decode_batch(cls, loc, codec, 0.5, 10, False, seg_mask=torch.from_numpy(mask).cuda(), seg_filter=None)
    assert [[lane_key(l) for l in im] for im in plain] == [[lane_key(l) for l in im] for im in off]
    one = LC.decode(cls[1], loc[1], codec, 0.5, 10, False)
    assert [lane_key(l) for l in one] == [lane_key(l) for l in plain[1]]
    # and they are the raw kernel's survivors
    X = torch.empty((2, 16, 16), device=cls.device)
    prob = torch.empty((2, 16), device=cls.device)
    ints = torch.empty((4, 2, 16), device=cls.device, dtype=torch.int32)
    counts = torch.empty((2,), device=cls.device, dtype=torch.int32)
    lib().call("hn_lane_decode_nms", cls.data_ptr(), loc.data_ptr(), 2, 128, 128, 32, 16, 0.5, 10.0, 0, 100.0, X.data_ptr(), prob.data_ptr(),
               ints[0].data_ptr(), ints[1].data_ptr(), ints[2].data_ptr(), ints[3].data_ptr(), counts.data_ptr())
    Xh, ph, (st, en, order, keep), ch = X.cpu().numpy(), prob.cpu().numpy(), ints.cpu().numpy(), counts.cpu().numpy()
    for n in range(2):
        want = [(float(ph[n, order[n, j]]), int(st[n, order[n, j]]), int(en[n, order[n, j]])) for j in range(ch[n]) if keep[n, j]]
        assert [(float(l.prob), l.start_pos, l.end_pos) for l in plain[n]] == want
        for l in plain[n]:
            a = int(l.ay // 32) * 4 + int(l.ax // 32)
            assert [float(p.x) for p in l.lane] == Xh[n, a, l.start_pos:l.end_pos].tolist()


def test_decode_batch_with_the_filter_equals_the_reference(synthetic_head):
    from multitask_hydranet_amd import lane_codec as LC
    codec, cls, loc, mask = synthetic_head
    plain = LC.decode_batch(cls, loc, codec, 0.5, 10, False)
    assert all(len(im) >= 3 for im in plain)
    md = torch.from_numpy(mask).cuda()
    logits = torch.nn.functional.one_hot(md, 5).permute(0, 3, 1, 2).float()
    for f in (LC.LaneSegFilter(), LC.LaneSegFilter(top_k=3), LC.LaneSegFilter(lane_class=1, min_ratio=0.5, line_width=9)):
        want = [R.filter_lanes(plain[n], mask[n], 128, 128, f) for n in range(2)]
        for seg in (md, logits):
            lanes, stats = LC.decode_batch(cls, loc, codec, 0.5, 10, False, seg_mask=seg, seg_filter=f, return_stats=True)
            for n in range(2):
                assert stats[n] == want[n][1], (f, n)
                assert [lane_key(l) for l in lanes[n]] == [lane_key(l) for l in want[n][0]], (f, n)
        only = LC.decode_batch(cls, loc, codec, 0.5, 10, False, seg_mask=md, seg_filter=f)           # without the statistics: the lanes alone
        assert [[lane_key(l) for l in im] for im in only] == [[lane_key(l) for l in w[0]] for w in want]
        l1, s1 = LC.decode(cls[1], loc[1], codec, 0.5, 10, False, seg_mask=md[1], seg_filter=f, return_stats=True)
        assert s1 == want[1][1] and [lane_key(l) for l in l1] == [lane_key(l) for l in want[1][0]]
    for n in range(2):                                                   # the deploy constants drop some and keep some
        verdicts = [s["kept"] for s in R.filter_lanes(plain[n], mask[n], 128, 128, LC.LaneSegFilter())[1]]
        assert any(verdicts) and not all(verdicts), (n, verdicts)
    with pytest.raises(ValueError):
        LC.decode_batch(cls, loc, codec, 0.5, 10, False, seg_mask=md[:, :64], seg_filter=LC.LaneSegFilter())


# ---- demo ------------------------------------------------------------------------------------------------------------------------------
H0, W0 = 270, 480


@pytest.fixture(scope="module")
def demo():
    """the tiny cfg with its recorded weights.  Those weights give every anchor rel_up = -0.19 and rel_down = 0.10 on any frame (at most one
    point per anchor), so no threshold lets a lane through: the two range biases of the lane head's last layer are raised (9 points up,
    3 down), nothing else is touched.  The recorded seg head answers class 4 everywhere, so the filters below name class 4 as well as 2."""
    from multitask_hydranet_amd.demo import Demo
    d = Demo(load_cfg("hydranet_tiny.yml"), fold_batchnorm=False)
    sd = tiny_state(load_npz("tiny_hydranet.npz"))
    sd["laneheader.conv_up_conv.3.bias"] = sd["laneheader.conv_up_conv.3.bias"].clone()
    sd["laneheader.conv_up_conv.3.bias"][0] += 9.0                       # predict_loc = [down offsets, rel_down | rel_up, up offsets]
    sd["laneheader.conv_down_conv.3.bias"] = sd["laneheader.conv_down_conv.3.bias"].clone()
    sd["laneheader.conv_down_conv.3.bias"][-1] += 3.0
    d.net.load_state_dict(sd)
    d.net.eval().prepare_inference()
    d.lane_conf, d.det_conf = 0.3, 0.3                                   # thresholds that let the tiny model produce lanes and boxes
    return d


def packed(frames, dev):
    n = len(frames)
    return {"data": torch.from_numpy(np.ascontiguousarray(frames).reshape(-1)).to(dev), "offsets": H0 * W0 * 3 * np.arange(n, dtype=np.int64),
            "shapes": np.array([[H0, W0]] * n, np.int64)}


def by_hand(demo, frames, f):
    """forward, the unfiltered decode, the arg-max map, then the reference's filter on the host -> (lanes, stats, unfiltered lanes)"""
    from multitask_hydranet_amd.preprocess import preprocess_bgr
    net = demo.net
    with torch.no_grad():
        out = net(preprocess_bgr(torch.from_numpy(np.ascontiguousarray(frames)).to(demo.device), (demo.net_h, demo.net_w), device=demo.device))
        mask = demo._seg_mask(out["seg"]).cpu().numpy()
        sets = net.laneheader.decode_batch(out["lane"]["predict_cls"], out["lane"]["predict_loc"], demo.lane_coder, demo.lane_conf, demo.lane_nms, False)
    to_org = lambda s: net.laneheader.scale_to_org(s, demo.net_w, demo.net_h, W0, H0)["Lines"]
    got = [R.filter_lanes(s, mask[n], demo.net_h, demo.net_w, f) for n, s in enumerate(sets)]
    return [to_org(g[0]) for g in got], [g[1] for g in got], [to_org(s) for s in sets]


def test_demo_filters_the_lanes_it_draws(demo):
    from multitask_hydranet_amd import demo as DM
    from multitask_hydranet_amd.lane_codec import LaneSegFilter
    frames = DM.synthetic_frames(2, H0, W0, seed=4)
    for conf in (0.3, 0.1, 0.03, 0.011):                                 # lowered until the tiny model's unfiltered decode finds lanes
        demo.lane_conf = conf
        found = [len(l) for l in by_hand(demo, frames, LaneSegFilter())[2]]
        print("demo lane filter: lane_conf %.3f -> %s unfiltered lanes" % (conf, found))
        if min(found) > 0:
            break
    plain = demo.process_device_batch(packed(frames, demo.device))
    assert "lane_filter" not in plain
    explicit_off = demo.process_device_batch(packed(frames, demo.device), lane_seg_filter=False)
    assert explicit_off["jpeg"] == plain["jpeg"] and explicit_off["lanes"] == plain["lanes"]
    seen = set()
    custom = [LaneSegFilter(lane_class=4), LaneSegFilter(top_k=1, lane_class=4, min_ratio=0.3, line_width=7)]
    for arg, f in [(True, LaneSegFilter())] + [(c, c) for c in custom]:
        lanes, stats, unfiltered = by_hand(demo, frames, f)
        assert sum(len(l) for l in unfiltered) > 0 and unfiltered == plain["lanes"], "the thresholds let no lane through: nothing to filter"
        r = demo.process_device_batch(packed(frames, demo.device), lane_seg_filter=arg)
        assert r["lanes"] == lanes and r["lane_filter"] == stats
        assert len(r["jpeg"]) == 2 and all(j[:2] == b"\xff\xd8" for j in r["jpeg"])
        if lanes == unfiltered:                                          # nothing dropped: the very same drawing
            assert r["jpeg"] == plain["jpeg"]
        seen |= {s["kept"] for im in stats for s in im}
        for n in range(2):                                               # every frame alone
            l1, s1, _ = by_hand(demo, frames[n:n + 1], f)
            r1 = demo.process_device(packed(frames[n:n + 1], demo.device), lane_seg_filter=arg)
            assert r1["lanes"] == l1 and r1["lane_filter"] == s1
        h = demo.process(frames[0], lane_seg_filter=arg)
        l1, s1, _ = by_hand(demo, frames[:1], f)
        assert h["lanes"] == l1 and h["lane_filter"] == s1
    print("demo lane filter verdicts seen: %s" % sorted(seen))
    assert seen == {False, True}                                         # lanes were dropped (class 2 is nowhere) and kept (class 4 is everywhere)
    # the constructor's switch is the calls' default
    demo.lane_seg_filter = demo._lane_filter(True, None)
    try:
        r = demo.process_device_batch(packed(frames, demo.device))
        assert r["lane_filter"] == by_hand(demo, frames, LaneSegFilter())[1]
    finally:
        demo.lane_seg_filter = None


def test_demo_refuses_a_cfg_without_the_seg_head():
    from multitask_hydranet_amd.demo import Demo
    cfg = load_cfg("hydranet_tiny.yml")
    cfg["train"]["train_seg"] = False
    with pytest.raises(ValueError):
        Demo(cfg, lane_seg_filter=True)


def test_command_line_writes_the_statistics(tmp_path):
    import json
    import os
    from multitask_hydranet_amd import demo as DM
    np.save(tmp_path / "frames.npy", DM.synthetic_frames(2, H0, W0, seed=4))
    cfg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cfgs", "hydranet_tiny.yml")
    base = ["--cfg", cfg, "--frames", str(tmp_path / "frames.npy")]
    off = DM.main(base + ["--out", str(tmp_path / "off")])
    on = DM.main(base + ["--out", str(tmp_path / "on"), "--lane-seg-filter", "--lane-top-k", "3", "--lane-seg-class", "4"])
    assert all("lane_filter" not in e for e in off) and all(isinstance(e["lane_filter"], list) and len(e["lane_filter"]) <= 3 for e in on)
    assert all(e["lanes"] == sum(s["kept"] for s in e["lane_filter"]) for e in on)
    assert [e["lane_filter"] for e in json.load(open(tmp_path / "on" / "results.json"))] == [e["lane_filter"] for e in on]
    assert np.array_equal(np.load(tmp_path / "on" / "frame_0000.npy"), np.load(tmp_path / "off" / "frame_0000.npy"))   # --frames draws no lanes
