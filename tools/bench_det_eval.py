"""COCO box mAP on the device (det_eval.CocoBoxEvaluator, hn_coco.hip) on a synthetic validation set: 5 000 images at 1920 x 1080,
0..40 GTs per image over 9 classes (areas straddling 32^2 and 96^2), ~100 detections per image (jittered GTs and false positives, scores
quantised to 1/64 so ties occur; tests/coco_eval_ref.synthetic_set).
  (a) device time (HIP events) of all update() calls (--batch images each, the validation loop's shape) plus compute(), after a warm-up
      run; the host packing is inside the window, as in HydraTrainer.valid;
  (b) the device time of the kernels alone is left to a kernel trace (rocprofv3 --kernel-trace --stats);
  (c) the wall time of the fp64 restatement (tests/coco_eval_ref.py) on the same data, and whether both agree (precision / recall
      bitwise).  --skip-ref leaves (c) out.
Prints one line per measurement and a final JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=5000)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--skip-ref", action="store_true")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--dump", default="", help="write precision / recall of the device and the restatement to this .npz")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_det_eval.py measures the MI355X"
    import __graft_entry__ as g
    g.build()
    from multitask_hydranet_amd.det_eval import CocoBoxEvaluator
    from tests.coco_eval_ref import coco_eval_ref, synthetic_set

    gt, res = synthetic_set(args.images, args.seed, dets_per_image=130)
    print("set: %d images, %d GTs, %d detections" % (len(gt["images"]), len(gt["annotations"]), len(res)))
    ids = np.asarray([r["image_id"] for r in res])
    order = np.argsort(ids, kind="stable")
    cols = (ids[order], np.asarray([r["category_id"] for r in res])[order], np.asarray([r["bbox"] for r in res])[order],
            np.asarray([r["score"] for r in res])[order])
    cuts = np.searchsorted(cols[0], np.r_[np.arange(1, args.images + 1, args.batch), args.images + 1])     # image ids 1..images
    ev = CocoBoxEvaluator(gt, device="cuda:0")

    def run():
        ev.reset()
        for a, b in zip(cuts[:-1], cuts[1:]):
            ev.update_records(*(c[a:b] for c in cols))
        return ev.compute()

    out = run()                                               # warm-up (code objects, allocator)
    torch.cuda.synchronize()
    times, walls = [], []
    for _ in range(args.repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        out = run()
        e1.record()
        e1.synchronize()
        walls.append(time.perf_counter() - t0)
        times.append(e0.elapsed_time(e1))
    dev_ms = float(np.median(times))
    print("device: all updates + compute %.2f ms (HIP events, median of %d; host wall %.1f ms)" % (dev_ms, args.repeats, 1e3 * np.median(walls)))
    print("stats", np.round(out["stats"], 4).tolist())
    result = dict(images=args.images, detections=len(res), device_ms=dev_ms, wall_ms=1e3 * float(np.median(walls)))
    if not args.skip_ref:
        t0 = time.perf_counter()
        ref = coco_eval_ref(gt, res)
        ref_s = time.perf_counter() - t0
        same = bool(np.array_equal(ref["precision"], out["precision"]) and np.array_equal(ref["recall"], out["recall"]))
        print("restatement: %.1f s wall, precision / recall bitwise equal: %s" % (ref_s, same))
        result.update(ref_s=ref_s, bitwise_equal=same)
        if args.dump:
            np.savez(args.dump, precision=out["precision"], recall=out["recall"], ref_precision=ref["precision"], ref_recall=ref["recall"])
    print(json.dumps(result))


if __name__ == "__main__":
    main()
