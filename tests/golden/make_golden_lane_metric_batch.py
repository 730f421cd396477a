#!/usr/bin/env python3
"""Generate tests/golden/lane_metric_batch.json by running the REFERENCE's head_lane/lane_metric.py (spline_interp, calc_iou, LaneMetric)
on one ragged batch of 12 synthetic images (build container only; the reference is imported with throw-away shims as in make_golden.py:
cv2.line = the oracle's restated thick-line rasteriser, so the fill rule is SELF-CONSISTENT ONLY, parity with OpenCV itself unpinned).

Per image: the pair LaneMetric takes (pr_result / gt_result with Shape), and for lane_width 30 and 10 the full IoU matrix of calc_iou over
(non-empty ground truths) x (all non-empty predictions, whatever their score); once per image the int()-truncated samples of every such
lane, stored as the first sample followed by the steps between neighbours (np.cumsum restores them).  Per lane width and thresh_list
([0.5] and [0.3, 0.5, 0.7]): every handler's result_record and summary(), and LaneMetric.summary().
The batch covers: three frame sizes (96 x 160, 360 x 640, 250 x 333: no multiple of a tile); a lane of one point, of two points, one with a
repeated point (h = 0); a lane leaving the frame on the left (negative x) and one at the bottom; ground truth without prediction and the
reverse; an image without lanes; a near-vertical and a near-horizontal lane; two lanes crossing inside one tile; predictions with and
without `score`.
Run:  python tests/golden/make_golden_lane_metric_batch.py"""
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference/model"
sys.dont_write_bytecode = True

SIZES = {"s": (96, 160), "m": (360, 640), "o": (250, 333)}          # (height, width)
WIDTHS = (30, 10)
THRESH_LISTS = ([0.5], [0.3, 0.5, 0.7])


def _reference():
    d = tempfile.mkdtemp(prefix="refstubs_")
    open(os.path.join(d, "cv2.py"), "w").write(
        "import sys\nsys.path.insert(0, %r)\nfrom oracle.hydranet_oracle import cv2_line as line\n"
        "def bitwise_or(a, b):\n    return a | b\n" % ROOT)
    sys.path.insert(0, d)
    sys.path.insert(0, REF)
    from head_lane import lane_metric as LM
    return LM


def lane(x0, y0, x1, y1, n, bend=0.0, jitter=0.0, rs=None):
    """n points from (x0, y0) to (x1, y1), bowed sideways by `bend` pixels"""
    t = np.linspace(0.0, 1.0, n)
    xs = x0 + (x1 - x0) * t + bend * 4 * t * (1 - t)
    ys = y0 + (y1 - y0) * t
    if jitter:
        xs = xs + jitter * rs.randn(n)
    return [{"x": float(np.round(x, 3)), "y": float(np.round(y, 3))} for x, y in zip(xs, ys)]


def shifted(ln, dx, dy=0.0):
    return [{"x": p["x"] + dx, "y": p["y"] + dy} for p in ln]


def images():
    rs = np.random.RandomState(7)
    out = []

    def image(size, gts, prs):
        h, w = SIZES[size]
        shape = {"width": w, "height": h}
        out.append(dict(pr_result={"Lines": prs, "Shape": shape}, gt_result={"Lines": gts, "Labels": [1] * len(gts), "Shape": shape}))

    # 0: small frame, three lanes, predictions close / off / far
    g = [lane(20, 95, 60, 5, 5, bend=4), lane(80, 95, 85, 5, 6, bend=-3), lane(140, 95, 100, 10, 4, bend=6)]
    image("s", g, [{"score": 0.9, "points": shifted(g[0], 2.0)}, {"score": 0.6, "points": shifted(g[1], 9.0)},
                   {"score": 0.4, "points": shifted(g[2], -30.0)}])
    # 1: near-vertical, near-horizontal, two lanes crossing inside the tile [128, 192) x [192, 256)
    g = [lane(300.2, 355, 301.1, 20, 7), lane(30, 180.3, 600, 182.9, 8), lane(135, 250, 185, 200, 3), lane(135, 200, 185, 250, 3)]
    image("m", g, [{"score": 0.8, "points": shifted(g[0], 3.0)}, {"score": 0.55, "points": shifted(g[1], 0.0, 4.0)},
                   {"score": 0.35, "points": shifted(g[2], 1.0, 1.0)}, {"score": 0.95, "points": shifted(g[3], -2.0, 5.0)}])
    # 2: odd frame; one lane leaves on the left with negative x, one below the bottom edge
    g = [lane(60, 240, -45.5, 120, 6, bend=10), lane(200, 310.5, 170, 60, 7, bend=-8), lane(300, 245, 250, 40, 5)]
    image("o", g, [{"score": 0.7, "points": shifted(g[0], 4.0)}, {"score": 0.2, "points": shifted(g[1], -3.0, 2.0)}])
    # 3: ground truth without prediction; 4: the reverse; 5: nothing
    image("s", [lane(30, 90, 70, 10, 5), lane(120, 90, 90, 10, 5)], [])
    image("s", [], [{"score": 0.9, "points": lane(40, 92, 75, 12, 4)}, lane(110, 92, 95, 12, 3)])
    image("s", [], [])
    # 6: a lane of one point, of two points, one with a repeated point; predictions without score
    rep = lane(150, 240, 180, 60, 6, bend=5)
    rep.insert(3, dict(rep[2]))
    g = [[{"x": 50.5, "y": 120.25}], lane(90, 245, 120, 30, 2), rep]
    image("o", g, [shifted(g[1], 5.0), shifted(rep, -4.0), [{"x": 52.0, "y": 118.0}], {"score": 0.65, "points": shifted(g[1], -11.0)}])
    # 7: scores either side of every threshold, with and without score
    g = [lane(100 + 130 * j, 350, 220 + 60 * j, 40, 8, bend=12 - 6 * j, jitter=1.5, rs=rs) for j in range(4)]
    image("m", g, [{"score": 0.25, "points": shifted(g[0], 3.0)}, {"score": 0.45, "points": shifted(g[1], 5.0)},
                   {"score": 0.65, "points": shifted(g[2], 6.0)}, shifted(g[3], 2.0), {"score": 0.75, "points": lane(600, 340, 420, 100, 5)}])
    # 8: empty entries on both sides (dropped), a prediction below every threshold
    g = [lane(25, 94, 50, 8, 4), [], lane(130, 94, 110, 8, 5, bend=-5)]
    image("s", g, [{"score": 0.1, "points": shifted(g[0], 1.0)}, {"score": 0.9, "points": []}, {"score": 0.8, "points": shifted(g[2], 6.0)}])
    # 9: predictions near the IoU threshold
    g = [lane(40, 248, 120, 30, 6, bend=7), lane(280, 248, 200, 30, 6, bend=-7)]
    image("o", g, [{"score": 0.6, "points": shifted(g[0], 8.0)}, {"score": 0.6, "points": shifted(g[1], -10.0)},
                   {"score": 0.31, "points": shifted(g[1], 3.0)}])
    # 10: more predictions than ground truths: the assignment has to choose
    g = [lane(150, 358, 280, 60, 9, bend=15, jitter=1.0, rs=rs), lane(480, 358, 350, 60, 9, bend=-15, jitter=1.0, rs=rs)]
    image("m", g, [{"score": 0.9, "points": shifted(g[0], 6.0)}, {"score": 0.52, "points": shifted(g[0], -3.0)},
                   {"score": 0.71, "points": shifted(g[1], 4.0)}, {"score": 0.33, "points": shifted(g[1], 1.0)}])
    # 11: small frame, lanes partly outside on every side
    g = [lane(-20, 60, 60, -15, 4), lane(150, 110, 120, 30, 4, bend=5)]
    image("s", g, [shifted(g[0], 3.0, 1.0), {"score": 0.5, "points": shifted(g[1], -5.0)}])
    return out


def eval_lanes(pair):
    """what LaneMetricCore keeps before the score test: non-empty ground truths, non-empty predictions (all scores)"""
    gts = [ln for ln in pair["gt_result"]["Lines"] if len(ln) > 0]
    prs = [ln["points"] if "score" in ln else ln for ln in pair["pr_result"]["Lines"]]
    return gts, [ln for ln in prs if len(ln) > 0]


def main():
    LM = _reference()
    imgs = images()
    out = {"images": imgs, "samples": [], "iou": {}, "results": {}}
    for pair in imgs:
        gts, prs = eval_lanes(pair)
        lanes = []
        for ln in gts + prs:
            xy = np.array([[int(p["x"]), int(p["y"])] for p in LM.spline_interp(lane=ln, step_t=1)], dtype=np.int64).reshape(-1, 2)
            d = np.diff(xy, axis=0, prepend=np.zeros((1, 2), np.int64))       # first sample, then steps: cumsum gives the samples back
            lanes.append({"dx": d[:, 0].tolist(), "dy": d[:, 1].tolist()})
        out["samples"].append(lanes)
    for lw in WIDTHS:
        mats = []
        for pair in imgs:
            gts, prs = eval_lanes(pair)
            hp = dict(eval_height=pair["gt_result"]["Shape"]["height"], eval_width=pair["gt_result"]["Shape"]["width"], lane_width=lw)
            mats.append([[float(LM.calc_iou(g, p, hp)) for p in prs] for g in gts])
        out["iou"][str(lw)] = mats
        for tl in THRESH_LISTS:
            m = LM.LaneMetric(method="f1_measure", iou_thresh=0.5, lane_width=lw, thresh_list=tl)
            m.reset()
            m(output=imgs)
            key = "%d|%s" % (lw, ",".join("%g" % t for t in tl))
            out["results"][key] = {"handlers": [{"records": h.result_record, "summary": h.summary()} for h in m.metric_handlers],
                                   "summary": m.summary()}
            print(key, [h.summary() for h in m.metric_handlers])
    path = os.path.join(HERE, "lane_metric_batch.json")
    json.dump(out, open(path, "w"), separators=(",", ":"))
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
