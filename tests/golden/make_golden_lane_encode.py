#!/usr/bin/env python3
"""Generate tests/golden/lane_encode_kats.npz by running the REFERENCE's lane encoder (head_lane/lane_codec.py LaneCodec.encode_lane,
numpy + scipy) on CPU, followed by the dataset's scale-invariance division (dataset/dataloader.py:346-352), on synthetic annotations.

Per geometry `<g>/`: meta int64 [W, H, stride, P, interpolate, scale_invariance, cfg interval]; annot = the raw annotation JSON per image;
src int64 [n, 2] = (org width, org height); gt_cls fp32 [n, F, 2]; gt_loc fp32 [n, F, 2P+2] (after the division when scale_invariance).
Coordinates are continuous random values; no anchor of the fixture has tied candidates with different rows (asserted: the reference's
pick among exact ties is numpy argsort's, which is not always the first).
Run:  python tests/golden/make_golden_lane_encode.py"""
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/model"
sys.dont_write_bytecode = True

GEOMS = [  # name, W, H, interpolate, scale_invariance, org (w, h), images
    ("g640i", 640, 640, True, True, (2560, 1440)),
    ("g640n", 640, 640, False, True, (2560, 1440)),
    ("g512x1024", 1024, 512, True, False, (1920, 1080)),
    ("g128", 128, 128, True, True, (1280, 720)),
]
STRIDE, INTERVAL = 32, 8


def _reference():
    d = tempfile.mkdtemp(prefix="refstubs_")
    open(os.path.join(d, "cv2.py"), "w").write("")            # lane_codec_utils imports cv2 for drawing only
    sys.path.insert(0, d)
    sys.path.insert(0, REF)
    import head_lane.lane_codec as lc
    return lc


def _num(g, v, as_str):
    v = float(np.round(v, 3))
    return repr(v) if as_str else v


def _lane(g, ow, oh, n, x0=None, y0=None, x1=None, y1=None, as_str=None, top_down=None):
    """a smooth lane of n points from (x0, y0) (bottom) to (x1, y1) (top), in source pixels"""
    x0 = g.uniform(-0.1 * ow, 1.1 * ow) if x0 is None else x0
    y0 = g.uniform(0.75 * oh, 1.02 * oh) if y0 is None else y0
    x1 = g.uniform(0.3 * ow, 0.7 * ow) if x1 is None else x1
    y1 = g.uniform(0.3 * oh, 0.6 * oh) if y1 is None else y1
    bend = g.uniform(-0.05, 0.05) * ow
    t = np.sort(g.uniform(0, 1, n)) if n > 2 else np.array([0.0, 1.0])[:n]
    t[0] = 0.0
    if n > 1:
        t[-1] = 1.0
    xs = x0 + (x1 - x0) * t + bend * t * (1 - t) * 4
    ys = y0 + (y1 - y0) * t
    as_str = bool(g.integers(2)) if as_str is None else as_str
    pts = [{"x": _num(g, x, as_str), "y": _num(g, y, as_str)} for x, y in zip(xs, ys)]
    top_down = bool(g.integers(2)) if top_down is None else top_down
    return pts[::-1] if top_down else pts


def _random_image(g, ow, oh, nl=None):
    nl = int(g.integers(2, 7)) if nl is None else nl
    return {"Lines": [_lane(g, ow, oh, int(g.integers(4, 40))) for _ in range(nl)]}


def _edge_images(g, ow, oh, W, H):
    sx, sy = ow / W, oh / H                                  # target pixels -> source pixels
    imgs = [{"Lines": []}]
    # "nan" points and raw-duplicate y ("10" / "10.0" are two points of one float y; a numeric duplicate is dropped on the raw value)
    a = _lane(g, ow, oh, 12, as_str=True, top_down=False)
    a.insert(3, {"x": "nan", "y": a[3]["y"]})
    a.insert(6, {"x": a[6]["x"], "y": "nan"})
    yv = float(a[8]["y"])
    a.insert(9, {"x": repr(float(a[8]["x"]) + 7.25), "y": repr(yv) + "0"})
    b = _lane(g, ow, oh, 10, as_str=False, top_down=True)
    b.insert(4, {"x": b[4]["x"] + 3.5, "y": b[4]["y"]})
    c = [{"x": "500.5", "y": "10"}, {"x": "520.25", "y": "10.0"}]            # collapses to one float y: no lane
    imgs.append({"Lines": [a, b, c]})
    # 1, 2, 3, 4 and 200 points
    imgs.append({"Lines": [_lane(g, ow, oh, 1), _lane(g, ow, oh, 2), _lane(g, ow, oh, 3), _lane(g, ow, oh, 4),
                           _lane(g, ow, oh, 200, top_down=False)]})
    # short lanes: mid image (the extension rescues them with interpolate) and at the very bottom (dropped in both modes)
    imgs.append({"Lines": [_lane(g, ow, oh, 3, x0=0.4 * ow, y0=0.5 * oh + 3.1 * sy, x1=0.41 * ow, y1=0.5 * oh),
                           _lane(g, ow, oh, 4, x0=0.6 * ow, y0=(H - 0.3) * sy, x1=0.62 * ow, y1=(H - 3.7) * sy),
                           _lane(g, ow, oh, 6)]})
    # first point below the image (extrapolation; k=1 fits of 3 kept points), lanes leaving the left and the right edge
    imgs.append({"Lines": [_lane(g, ow, oh, 2, x0=0.3 * ow, y0=(H + 50.3) * sy, x1=0.31 * ow, y1=(H - 2.4) * sy),
                           _lane(g, ow, oh, 5, x0=0.7 * ow, y0=1.3 * oh, x1=0.55 * ow, y1=0.4 * oh),
                           _lane(g, ow, oh, 8, x0=-0.2 * ow, y0=0.95 * oh, x1=0.25 * ow, y1=0.45 * oh),
                           _lane(g, ow, oh, 8, x0=1.15 * ow, y0=0.9 * oh, x1=0.8 * ow, y1=0.4 * oh),
                           _lane(g, ow, oh, 6, x0=-3.7 * sx, y0=0.99 * oh, x1=0.2 * ow, y1=0.5 * oh)]})
    # crossing lanes (several candidates per anchor) and a duplicated lane
    l1 = _lane(g, ow, oh, 9, x0=0.2 * ow, y0=oh, x1=0.7 * ow, y1=0.35 * oh)
    l2 = _lane(g, ow, oh, 9, x0=0.75 * ow, y0=oh, x1=0.25 * ow, y1=0.35 * oh)
    l3 = _lane(g, ow, oh, 9, x0=0.45 * ow, y0=0.98 * oh, x1=0.5 * ow, y1=0.3 * oh)
    imgs.append({"Lines": [l1, l2, l3, list(l3)]})
    # >= 8 lanes
    imgs.append(_random_image(g, ow, oh, nl=9))
    return imgs


def main():
    lc = _reference()
    seen = []
    orig = lc.get_lane_loc_list

    def spy(dist, loc, h, w):
        out = orig(dist, loc, h, w)
        seen.append(out)
        return out

    lc.get_lane_loc_list = spy
    g = np.random.default_rng(20261015)
    rec = {}
    for name, W, H, interp, si, (ow, oh) in GEOMS:
        P = int(H / INTERVAL)
        codec = lc.LaneCodec(input_width=W, input_height=H, anchor_stride=STRIDE, points_per_line=P, do_interpolate=interp,
                             anchor_lane_num=1, scale_invariance=si)
        imgs = _edge_images(g, ow, oh, W, H) if W >= 512 else []
        imgs += [_random_image(g, ow, oh) for _ in range(6 if W >= 512 else 3)]
        cls_l, loc_l, annots, srcs = [], [], [], []
        for k, obj in enumerate(imgs):
            js = json.dumps(obj)
            seen.clear()
            gt_type, gt_loc = codec.encode_lane(lane_object=json.loads(js), org_width=ow, org_height=oh)
            for locs, dists in seen:
                if len(dists) > 1:
                    d = [q[2] for q in dists]
                    best = min(d)
                    rows = [np.asarray(locs[i], np.float64) for i in range(len(d)) if d[i] == best]
                    assert all(np.array_equal(rows[0], r) for r in rows), (name, k, "tied candidates with different rows")
            if si:
                gt_loc[:, P + 2:2 * P + 2] /= INTERVAL
                gt_loc[:, :P] /= INTERVAL
            cls_l.append(gt_type.astype(np.float32))
            loc_l.append(gt_loc.astype(np.float32))
            annots.append(js)
            srcs.append((ow, oh))
        rec[name + "/meta"] = np.array([W, H, STRIDE, P, int(interp), int(si), INTERVAL], np.int64)
        rec[name + "/annot"] = np.array(annots)
        rec[name + "/src"] = np.array(srcs, np.int64)
        rec[name + "/gt_cls"] = np.stack(cls_l)
        rec[name + "/gt_loc"] = np.stack(loc_l)
        print(name, len(imgs), "images", int((np.stack(cls_l)[:, :, 1] == 1).sum()), "lane anchors")
    np.savez_compressed(os.path.join(HERE, "lane_encode_kats.npz"), **rec)


if __name__ == "__main__":
    main()
