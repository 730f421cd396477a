"""Lane F1 on the device, per image against per batch (lane_metric.py): 64 synthetic 1080 x 1920 images with 4 ground
truths and 4 predictions of 11 points each (the lanes of tests/test_post_gpu.py's full-frame case, shifted per image; scores on both sides
of the thresholds), through LaneMetric(f1_measure, IoU 0.5, width 30, --thresh-list):
  (a) per image: LaneMetric(batched=False) -- host spline, masks in HBM, hn_lane_raster + hn_lane_iou and a blocking copy per image and
      threshold;
  (b) batched: LaneMetric(batched=True) -- --batch images per call (the validation loop's shape), hn_lane_metric_batch per call, one
      synchronisation in summary().
Both are timed with HIP events on the stream (the window holds the host work between the launches, as in HydraTrainer.valid) and with
the wall clock, after a warm-up run of each; the records of both must be equal.  The device time of the kernels alone is left to a kernel
trace (rocprofv3 --kernel-trace --stats).  Prints one line per measurement and a final JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def synthetic_pairs(images, seed, height=1080, width=1920):
    rs = np.random.RandomState(seed)
    shape = {"width": width, "height": height}
    out = []
    for k in range(images):
        gts = [[{"x": float(200 + 300 * j + 15 * i + 0.8 * i * i * (j - 2) + 3 * (k % 16)), "y": float(1070 - 90 * i)} for i in range(11)]
               for j in range(4)]
        prs = [{"score": float(rs.choice([0.35, 0.55, 0.75, 0.9])),
                "points": [{"x": p["x"] + float(rs.randint(-20, 20)), "y": p["y"]} for p in g]} for g in gts]
        out.append(dict(pr_result={"Lines": prs, "Shape": shape}, gt_result={"Lines": gts, "Labels": [1] * len(gts), "Shape": shape}))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--thresh-list", type=float, nargs="+", default=[0.5])
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_lane_metric.py measures the MI355X"
    import __graft_entry__ as g
    g.build()
    from multitask_hydranet_amd.lane_metric import LaneMetric

    pairs = synthetic_pairs(args.images, args.seed)
    chunks = [pairs[i:i + args.batch] for i in range(0, len(pairs), args.batch)]

    def run(batched):
        m = LaneMetric(method="f1_measure", iou_thresh=0.5, lane_width=30, thresh_list=args.thresh_list, batched=batched)
        m.reset()
        for c in chunks:
            m(output=c)
        return m.summary(), [h.result_record for h in m.metric_handlers]

    result = dict(images=args.images, batch=args.batch, thresh_list=args.thresh_list)
    outs = {}
    for name, batched in (("per_image", False), ("batched", True)):
        outs[name] = run(batched)                             # warm-up (code objects, allocator, pinned buffers)
        torch.cuda.synchronize()
        times, walls = [], []
        for _ in range(args.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            run(batched)
            e1.record()
            e1.synchronize()
            walls.append(time.perf_counter() - t0)
            times.append(e0.elapsed_time(e1))
        ev_ms, wall_ms = float(np.median(times)), 1e3 * float(np.median(walls))
        print("%-9s: %8.2f ms between HIP events, %8.2f ms wall (median of %d), %.3f ms wall per image"
              % (name, ev_ms, wall_ms, args.repeats, wall_ms / args.images))
        result[name + "_event_ms"], result[name + "_wall_ms"] = ev_ms, wall_ms
    same = outs["per_image"] == outs["batched"]
    print("f1 %.6f, records equal: %s" % (outs["batched"][0], same))
    result.update(f1=outs["batched"][0], records_equal=same, wall_speedup=result["per_image_wall_ms"] / result["batched_wall_ms"])
    print(json.dumps(result))


if __name__ == "__main__":
    main()
