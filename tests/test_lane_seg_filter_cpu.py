"""CPU: the lane filter by the seg head's marking class (lane_codec.LaneSegFilter, hn_lane_filter.hip) without a device -- the
library's exports and argument checks, the dataclass's validation, the unchanged default of decode / decode_batch, and the numpy
restatement (tests/lane_seg_filter_ref.py) pinned against the drawing reference's thick segment and against a count made by hand."""
import ctypes
import inspect

import numpy as np
import pytest

from tests import draw_ref
from tests import lane_seg_filter_ref as R


@pytest.fixture(scope="module")
def l():
    import __graft_entry__ as g
    g.build()
    from multitask_hydranet_amd._lib import lib
    return lib()


def test_header_declares_and_library_exports_the_filter(l):
    from multitask_hydranet_amd._lib import SO_PATH, SOURCES, parse_header
    sig = parse_header()
    dll = ctypes.CDLL(SO_PATH)
    assert "hn_lane_filter.hip" in SOURCES
    for name in ("hn_lane_seg_filter_ws_bytes", "hn_lane_seg_filter"):
        assert name in sig and hasattr(dll, name) and name in l.symbols()
    assert sig["hn_lane_seg_filter"][2] and not sig["hn_lane_seg_filter_ws_bytes"][2]              # the launcher takes the stream
    assert len(sig["hn_lane_seg_filter"][1]) == 23 and sig["hn_lane_seg_filter_ws_bytes"][0] is ctypes.c_long


def test_ws_bytes_is_monotone_and_refuses_what_is_out_of_range(l):
    q = lambda *a: l.query("hn_lane_seg_filter_ws_bytes", *a)
    base = q(2, 14, 80)
    assert base > 0 and q(3, 14, 80) > base and q(2, 15, 80) > base and q(2, 14, 81) > base
    assert q(1, 1, 1) > 0 and q(16, 64, 1024) > 0
    for bad in ((0, 14, 80), (-1, 14, 80), (2, 0, 80), (2, 65, 80), (2, 14, 0), (2, 14, 1025)):
        assert q(*bad) == -1, bad


def test_argument_checks_come_before_any_hip_call(l):
    f = l.raw("hn_lane_seg_filter")
    bufs = [ctypes.create_string_buffer(64) for _ in range(11)]         # never dereferenced: every call below is refused
    p = [ctypes.addressof(b) for b in bufs]
    ws = l.query("hn_lane_seg_filter_ws_bytes", 1, 14, 16)

    def call(**kw):
        a = dict(X=p[0], start=p[1], end=p[2], order=p[3], keep=p[4], counts=p[5], N=1, W=128, H=128, stride=32, ppl=16, interval=8,
                 mask=p[6], lane_class=2, line_width=20, min_ratio=0.01, top_k=14, ws=p[7], ws_bytes=ws, keep_out=p[8], stats=p[9],
                 n_sel=p[10])
        a.update(kw)
        return f(a["X"], a["start"], a["end"], a["order"], a["keep"], a["counts"], a["N"], a["W"], a["H"], a["stride"], a["ppl"], a["interval"],
                 a["mask"], a["lane_class"], a["line_width"], a["min_ratio"], a["top_k"], a["ws"], a["ws_bytes"], a["keep_out"], a["stats"],
                 a["n_sel"], None)

    for name in ("X", "start", "end", "order", "keep", "counts", "mask", "ws", "keep_out", "stats", "n_sel"):
        assert call(**{name: None}) == 1, name
    assert call(top_k=0) == 1 and call(top_k=65) == 1
    assert call(line_width=0) == 1 and call(line_width=-3) == 1
    assert call(H=100) == 1 and call(W=130) == 1                         # not a multiple of the stride
    assert call(ws_bytes=ws - 1) == 1 and call(ws_bytes=0) == 1
    assert call(N=0) == 1 and call(ppl=0) == 1 and call(interval=0) == 1 and call(stride=0) == 1


def test_lane_seg_filter_validation():
    from multitask_hydranet_amd.lane_codec import LaneSegFilter
    f = LaneSegFilter()
    assert (f.lane_class, f.line_width, f.min_ratio, f.top_k) == (2, 20, 0.01, 14)                  # hydranet_model.h:68-75
    assert LaneSegFilter(top_k=64, line_width=1, min_ratio=0.0, lane_class=0).top_k == 64
    for kw in (dict(top_k=0), dict(top_k=65), dict(top_k=2.5), dict(top_k=True), dict(line_width=0), dict(line_width=-1), dict(line_width=20.0),
               dict(lane_class=-1), dict(lane_class="2"), dict(min_ratio=float("nan")), dict(min_ratio=float("inf")), dict(min_ratio=None),
               dict(min_ratio="0.01")):
        with pytest.raises(ValueError):
            LaneSegFilter(**kw)
    with pytest.raises(Exception):
        f.top_k = 3                                                      # frozen


def test_default_is_the_old_code_path(monkeypatch):
    """seg_filter=None: decode / decode_batch hand on what they always did, and the filter's launcher is never reached"""
    import torch
    from multitask_hydranet_amd import lane_codec as LC
    for fn in (LC.decode, LC.decode_batch):
        sig = inspect.signature(fn)
        assert list(sig.parameters)[:6] == ["predict_cls", "predict_loc", "pointlane", "conf_thres", "nms_line_thres", "use_mean"]
        assert [sig.parameters[k].default for k in ("seg_mask", "seg_filter", "return_stats")] == [None, None, False]
    seen = []
    monkeypatch.setattr(LC, "_decode_batch", lambda *a, **kw: seen.append((a, kw)) or [["lanes"]])
    cls, loc = torch.zeros(1, 16, 2), torch.zeros(1, 16, 34)
    assert LC.decode_batch(cls, loc, "codec", 0.3, 80, False) == [["lanes"]]
    assert LC.decode(cls[0], loc[0], "codec", 0.3, 80, False) == ["lanes"]
    for a, kw in seen:
        assert a[2:] == ("codec", 0.3, 80, False) and kw == dict(seg_mask=None, seg_filter=None, return_stats=False)
    monkeypatch.undo()

    monkeypatch.setattr(LC, "_launch_seg_filter", lambda *a, **kw: pytest.fail("the filter was launched without a seg_filter"))
    codec = LC.LaneCodec(128, 128, 32, 16)
    # the filter's arguments are checked before anything touches the device
    with pytest.raises(ValueError):
        LC.decode_batch(cls, loc, codec, seg_filter=LC.LaneSegFilter())                             # no seg_mask
    with pytest.raises(ValueError):
        LC.decode_batch(cls, loc, codec, seg_mask=torch.zeros(1, 64, 128, dtype=torch.int64), seg_filter=LC.LaneSegFilter())
    with pytest.raises(ValueError):
        LC.decode_batch(cls, loc, codec, seg_mask=torch.zeros(2, 128, 128, dtype=torch.int64), seg_filter=LC.LaneSegFilter())
    with pytest.raises(ValueError):
        LC.decode_batch(cls, loc, codec, seg_mask=torch.zeros(1, 128, 128, dtype=torch.int32), seg_filter=LC.LaneSegFilter())
    with pytest.raises(ValueError):
        LC.decode_batch(cls, loc, codec, seg_mask=torch.zeros(1, 5, 128, 64), seg_filter=LC.LaneSegFilter())
    with pytest.raises(ValueError):
        LC.decode_batch(cls, loc, codec, seg_mask=torch.zeros(1, 128, 128, dtype=torch.int64), seg_filter={"top_k": 14})
    with pytest.raises(ValueError):
        LC.decode_batch(cls, loc, codec, return_stats=True)                                         # statistics of no filter
    with pytest.raises(ValueError):
        LC.decode_batch(cls, loc, LC.LaneCodec(128, 120, 8, 16), seg_mask=torch.zeros(1, 120, 128, dtype=torch.int64),
                        seg_filter=LC.LaneSegFilter())                                              # interval 7.5: no integer rows


def test_demo_refuses_the_filter_without_both_heads():
    from multitask_hydranet_amd.demo import Demo
    from multitask_hydranet_amd.lane_codec import LaneSegFilter
    d = Demo.__new__(Demo)                                               # the switch's own logic: no network, no device
    d.train_seg, d.train_lane = True, True
    assert d._lane_filter(None, None) is None and d._lane_filter(False, LaneSegFilter()) is None
    assert d._lane_filter(True, None) == LaneSegFilter() and d._lane_filter(None, LaneSegFilter(top_k=3)).top_k == 3
    assert d._lane_filter(LaneSegFilter(top_k=5), LaneSegFilter(top_k=3)).top_k == 5
    with pytest.raises(ValueError):
        d._lane_filter("yes", None)
    for seg, lane in ((False, True), (True, False)):
        d.train_seg, d.train_lane = seg, lane
        with pytest.raises(ValueError):
            d._lane_filter(True, None)
        assert d._lane_filter(None, None) is None


def test_reference_segment_is_the_drawing_reference_s(l):
    g = np.random.Generator(np.random.Philox(11))
    H, W = 72, 90
    ys, xs = np.mgrid[0:H, 0:W].astype(np.int64)
    cases = [(5, 5, 5, 5, 7), (10, 40, 60, 40, 20), (30, 2, 30, 60, 1), (-20, 10, 120, 50, 9)]
    for _ in range(60):
        x0, x1 = (int(v) for v in g.integers(-40, W + 40, 2))
        y0, y1 = (int(v) for v in g.integers(-40, H + 40, 2))
        cases.append((x0, y0, x1, y1, int(g.integers(1, 31))))
    painted = 0
    for x0, y0, x1, y1, t in cases:
        got = R.segment_mask(x0, y0, x1, y1, t, xs, ys)
        want = draw_ref.covers((0, x0, y0, x1, y1, t, 0), xs, ys)
        assert np.array_equal(got, want), (x0, y0, x1, y1, t)
        painted += int(got.sum())
    assert painted > 1000


def test_reference_against_a_count_by_hand():
    """128 x 128, one lane of the two points (10, 30) and (50, 30), width 20: the body's 41 x 21 pixels and two half discs of radius 10 (a
    disc of radius 10 holds 317 lattice points, 21 of them on its diameter column: (317 - 21) / 2 = 148 beyond either end)"""
    disc = sum(1 for x in range(-10, 11) for y in range(-10, 11) if x * x + y * y <= 100)
    assert disc == 317 and 41 * 21 + 2 * 148 == 1157
    m = R.lane_mask([(10, 30), (50, 30)], 128, 128, 20)
    assert int(m.sum()) == 1157
    # the same through the whole reference: a frame whose rows step sideways, so the lane's two points share y only in this direct call;
    # here the lane runs down the frame instead: (30, 127 - 8 p) for p = 2, 7 -> the same shape turned by 90 degrees
    H = W = 128
    X = np.zeros((1, 16, 16), np.float32)
    X[0, 3, 2:8] = 30.0
    start, end = np.zeros((1, 16), np.int32), np.zeros((1, 16), np.int32)
    start[0, 3], end[0, 3] = 2, 8
    order, keep, counts = np.zeros((1, 16), np.int32), np.zeros((1, 16), np.int32), np.array([1], np.int32)
    order[0, 0], keep[0, 0] = 3, 1
    for value, inter in ((2, 1157), (1, 0)):
        mask = np.full((1, H, W), value, np.int64)
        keep_out, stats, n_sel = R.seg_filter(X, start, end, order, keep, counts, W, H, 32, 16, 8, mask, 2, 20, 0.01, 14)
        assert n_sel.tolist() == [1] and stats[0, 0].tolist() == [0, 1157, inter, int(inter > 0)] and not stats[0, 1:].any()
        assert keep_out[0].tolist() == [int(inter > 0)] + [0] * 15


def test_reference_rounds_to_even_clamps_and_skips():
    assert R.lane_points(np.array([0.5, 1.5, 2.5, -0.5, 1e9, -1e9], np.float32), 0, 6, 100, 8) == \
        [(0, 99), (2, 91), (2, 83), (0, 75), (16383, 67), (-16383, 59)]
    assert R.lane_points(np.array([1.0, np.nan, 3.0], np.float32), 0, 3, 100, 8) is None
    assert R.lane_points(np.array([1.0, np.inf, 3.0], np.float32), 0, 3, 100, 8) is None
    assert R.lane_points(np.array([1.0, np.nan, 3.0], np.float32), 2, 3, 100, 8) is None              # a single point
    assert R.lane_points(np.array([np.nan, 2.0, 3.0], np.float32), 1, 3, 100, 8) == [(2, 91), (3, 83)]  # the NaN is outside the range
    assert not R.decide(0, 0, 0.01) and R.decide(2, 100, 0.01) and not R.decide(1, 100, 0.01)         # strict; 0 / 0 drops


def test_command_line_options_need_the_switch():
    from multitask_hydranet_amd import demo as DM
    for extra in (["--lane-top-k", "3"], ["--lane-seg-ratio", "0.1"], ["--lane-seg-width", "9"], ["--lane-seg-class", "1"]):
        with pytest.raises(SystemExit):
            DM.main(["--frames", "none.npy"] + extra)                    # refused while parsing: nothing is loaded
    with pytest.raises(ValueError):
        DM.main(["--frames", "none.npy", "--lane-seg-filter", "--lane-top-k", "0"])
