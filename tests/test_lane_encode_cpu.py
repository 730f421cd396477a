"""CPU: lane ground-truth encoding (LaneCodec.encode_lane + the dataset's division) -- the fp64 restatement (tests/lane_encode_ref.py)
against the reference's recorded outputs (tests/golden/lane_encode_kats.npz, make_golden_lane_encode.py), and the host packer of the device
path (lane_codec.parse_lane_object / pack_lanes) against the restatement's parse."""
import json

import numpy as np
import pytest

from tests.helpers import load_npz
from tests.lane_encode_ref import encode_ref, parse_lanes

GEOMS = ("g640i", "g640n", "g512x1024", "g128")


@pytest.fixture(scope="module")
def kats():
    return load_npz("lane_encode_kats.npz")


def _meta(z, g):
    W, H, S, P, ip, si, iv = (int(v) for v in z[g + "/meta"])
    return W, H, S, P, bool(ip), bool(si), iv


@pytest.mark.parametrize("g", GEOMS)
def test_restatement_reproduces_reference(kats, g):
    W, H, S, P, ip, si, iv = _meta(kats, g)
    for k, (a, src) in enumerate(zip(kats[g + "/annot"], kats[g + "/src"])):
        cls, loc = encode_ref(parse_lanes(str(a), W, H, src[0], src[1]), W, H, S, P, ip, si, iv)
        ec, el = kats[g + "/gt_cls"][k], kats[g + "/gt_loc"][k]
        assert np.array_equal(cls, ec), (g, k)
        assert np.array_equal(loc[:, P:P + 2], el[:, P:P + 2]), (g, k)
        assert np.abs(loc - el).max() <= 1e-5, (g, k)


def test_fixture_covers_the_edge_cases(kats):
    """the fixture is not all background and holds the branches the contract names"""
    W, H, S, P, ip, si, iv = _meta(kats, "g640n")
    annots = [json.loads(str(a)) for a in kats["g640n/annot"]]
    assert any(len(a["Lines"]) == 0 for a in annots)
    assert any(len(a["Lines"]) >= 8 for a in annots)
    assert any(p["x"] == "nan" or p["y"] == "nan" for a in annots for line in a["Lines"] for p in line)
    for g in GEOMS:
        assert (kats[g + "/gt_cls"][:, :, 1] == 1).sum() > 0, g
    # a lane starting below the image without interpolate: down counts beyond the image rows
    cnt = kats["g640n/gt_loc"][:, :, P]
    assert cnt.max() > 0


def test_packer_matches_restatement_parse(kats):
    from multitask_hydranet_amd.lane_codec import pack_lanes, parse_lane_object
    for g in GEOMS:
        W, H, S, P, ip, si, iv = _meta(kats, g)
        objs, srcs = [str(a) for a in kats[g + "/annot"]], [tuple(s) for s in kats[g + "/src"]]
        want = []
        for a, (ow, oh) in zip(objs, srcs):
            mine = parse_lane_object(json.loads(a), W, H, ow, oh)          # dict input
            ref = parse_lanes(a, W, H, ow, oh)
            assert len(mine) == len(ref), g
            for (x0, y0), (x1, y1) in zip(mine, ref):
                assert np.array_equal(x0, x1) and np.array_equal(y0, y1), g
            want.append(ref)
        pts, ints, nl = pack_lanes(objs, [dict(width=w, height=h) for w, h in srcs], W, H, H / P, ip, P)
        lane_off, img_lane = ints[:nl + 1], ints[nl + 1:]
        assert pts.dtype == np.float64 and ints.dtype == np.int32 and len(img_lane) == len(objs) + 1
        assert nl == sum(len(r) for r in want) and lane_off[-1] == len(pts)
        for i, ref in enumerate(want):
            lanes = range(img_lane[i], img_lane[i + 1])
            assert len(lanes) == len(ref)
            for l, (x, y) in zip(lanes, ref):
                seg = pts[lane_off[l]:lane_off[l + 1]]
                assert np.array_equal(seg[:, 0], x) and np.array_equal(seg[:, 1], y)


def test_packer_parse_rules():
    from multitask_hydranet_amd.lane_codec import parse_lane_object
    obj = {"Lines": [
        [{"x": "1", "y": "10"}, {"x": "2", "y": "10.0"}, {"x": "3", "y": "30"}, {"x": "nan", "y": "40"}, {"x": "4", "y": "10"}],
        [{"x": 5, "y": 50}, {"x": 6, "y": 50.0}, {"x": 7, "y": 20}],                  # numeric 50 == 50.0: one raw value
        [{"x": "1", "y": "10"}, {"x": "2", "y": "10.0"}],                               # one float y: dropped
        [{"x": 9, "y": 5}],
        [{"x": 1.5, "y": 1}, {"x": 2.5, "y": 3}, {"x": 3.5, "y": 2}],
        [{"x": "1", "y": "10"}, {"x": "2", "y": "20"}, {"x": "3", "y": "10.0"}],
    ]}
    lanes = parse_lane_object(json.dumps(obj), 100, 100, 200, 100)
    assert len(lanes) == 4
    # "10" and "10.0" are both kept, then the float y keeps the x of the first in list order ("1": no reversal, equal first two y)
    x, y = lanes[0]
    assert y.tolist() == [30.0, 10.0] and x.tolist() == [1.5, 0.5]
    # listed top-down -> reversed first, so the first of y = 10 is "3"
    x, y = lanes[3]
    assert y.tolist() == [20.0, 10.0] and x.tolist() == [1.0, 1.5]
    x, y = lanes[1]
    assert y.tolist() == [50.0, 20.0] and x.tolist() == [2.5, 3.5]
    x, y = lanes[2]
    assert y.tolist() == [3.0, 2.0, 1.0] and x.tolist() == [1.25, 1.75, 0.75]
    ref = parse_lanes(obj, 100, 100, 200, 100)
    assert all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(lanes, ref))


def test_packer_rejects_absurd_lanes():
    from multitask_hydranet_amd.lane_codec import pack_lanes
    long_lane = {"Lines": [[{"x": 0, "y": 0}, {"x": 9e6, "y": 1}, {"x": 0, "y": 2}]]}            # 1.8e7 spline samples
    with pytest.raises(ValueError):
        pack_lanes([long_lane], [(640, 640)], 640, 640, 8.0, True, 80)
    far_below = {"Lines": [[{"x": 100, "y": 5000}, {"x": 120, "y": 300}]]}
    pack_lanes([far_below], [(640, 640)], 640, 640, 8.0, True, 80)                     # with interpolate: fine
    with pytest.raises(ValueError):
        pack_lanes([far_below], [(640, 640)], 640, 640, 8.0, False, 80)
    with pytest.raises(ValueError):
        pack_lanes([long_lane], [(640, 640), (640, 640)], 640, 640, 8.0, True, 80)
    with pytest.raises(ValueError):
        pack_lanes([{"Lines": [[{"x": 0, "y": 0}, {"x": 3e7, "y": 1}]]}], [(640, 640)], 640, 640, 8.0, True, 80)


def test_encode_lane_other_anchor_lane_num_without_device():
    from multitask_hydranet_amd.lane_codec import LaneCodec
    c = LaneCodec(640, 640, 32, 80, do_interpolate=True, anchor_lane_num=2)
    assert c.encode_lane({"Lines": []}, 1280, 720) == (None, None)
    with pytest.raises(ValueError):
        c.encode_lanes([{"Lines": []}], [(1280, 720)])
