#!/usr/bin/env python3
"""Lane ground-truth encoding cost for one batch: the host packer (LaneCodec.encode_lanes' parse + pack, lane_codec.pack_lanes) and the
device encoder (hn_lane_encode, HIP events) timed separately, plus encode_lanes end to end (wall time to the synchronised result).
Default batch: N = 16 at 640x640 (interpolate, scale_invariance, stride 32, interval 8), 6 lanes of 50 points per image.
Prints one JSON line.   python tools/lane_encode_bench.py [--n 16] [--res 640x640] [--lanes 6] [--points 50] [--reps 50]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def batch(rng, n, lanes, points, ow=2560, oh=1440):
    objs = []
    for _ in range(n):
        lines = []
        for _ in range(lanes):
            x0, x1 = rng.uniform(-0.1, 1.1) * ow, rng.uniform(0.3, 0.7) * ow
            y0, y1 = rng.uniform(0.8, 1.0) * oh, rng.uniform(0.3, 0.6) * oh
            t = np.sort(rng.uniform(0, 1, points))
            xs = x0 + (x1 - x0) * t + rng.uniform(-0.05, 0.05) * ow * t * (1 - t) * 4
            ys = y0 + (y1 - y0) * t
            lines.append([{"x": "%.3f" % x, "y": "%.3f" % y} for x, y in zip(xs, ys)])
        objs.append(json.dumps({"Lines": lines}))
    return objs, [dict(width=ow, height=oh, channel=3)] * n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=16)
    ap.add_argument("--res", default="640x640", help="HxW")
    ap.add_argument("--lanes", type=int, default=6)
    ap.add_argument("--points", type=int, default=50)
    ap.add_argument("--reps", type=int, default=50)
    a = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    from multitask_hydranet_amd._lib import lib
    from multitask_hydranet_amd.lane_codec import LaneCodec, pack_lanes
    H, W = (int(v) for v in a.res.split("x"))
    P = H // 8
    codec = LaneCodec(W, H, 32, P, do_interpolate=True, anchor_lane_num=1, scale_invariance=True)
    objs, srcs = batch(np.random.default_rng(0), a.n, a.lanes, a.points)

    host = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        pts, ints, nl = pack_lanes(objs, srcs, W, H, codec.interval, True, P)
        host.append(time.perf_counter() - t0)

    dev = torch.device("cuda", 0)
    pts_d, ints_d = torch.from_numpy(pts).to(dev), torch.from_numpy(ints).to(dev)
    F = codec.feature_size
    cls = torch.empty((a.n, F, 2), device=dev)
    loc = torch.empty((a.n, F, 2 * P + 2), device=dev)
    ws = torch.empty((lib().query("hn_lane_encode_ws_bytes", nl, len(pts), W, H, 32, P),), device=dev, dtype=torch.uint8)

    def launch():
        lib().call("hn_lane_encode", pts_d.data_ptr(), ints_d.data_ptr(), ints_d.data_ptr() + 4 * (nl + 1), a.n, nl, len(pts), W, H, 32, P,
                   1, 1, 8.0, ws.data_ptr(), cls.data_ptr(), loc.data_ptr())
    for _ in range(5):
        launch()
    torch.cuda.synchronize()
    kern = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        launch()
        e1.record()
        e1.synchronize()
        kern.append(e0.elapsed_time(e1) * 1e-3)

    e2e = []
    for _ in range(a.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        c, l = codec.encode_lanes(objs, srcs, device=dev, div_interval=8)
        torch.cuda.synchronize()
        e2e.append(time.perf_counter() - t0)
    assert torch.equal(c, cls) and torch.equal(l, loc)
    ms = lambda v: round(float(np.median(v)) * 1e3, 4)
    print(json.dumps(dict(metric="lane_encode", n=a.n, res="%dx%d" % (H, W), lanes=a.lanes, points=a.points, lane_tasks=nl,
                          host_pack_ms=ms(host), kernel_ms=ms(kern), kernel_min_ms=round(min(kern) * 1e3, 4),
                          encode_lanes_end_to_end_ms=ms(e2e), reps=a.reps)))


if __name__ == "__main__":
    main()
