"""Detection NMS options (hn_det_postprocess_ex) at the big cfg's detection shape, next to the old entry point in the same
run: N = 16, the cfg's anchors at 512 x 1024 (A = 98 208), 9 classes, predictions from a seeded generator (scores sigmoid(N(-4, 1.5)),
regression N(0, 0.2)).  Two score thresholds, chosen from the scores so that about --few and about --many anchors per image pass; every
kind with max_det 0 and --max-det; the whole five-array pipeline (select, rank, suppression, gather) per call, timed with HIP events after
warm-up, the C entry points called directly on preallocated buffers.  The measurements are timed in alternating rounds of one process;
the median over the rounds is reported.  Prints one line per measurement and a final JSON line."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--few", type=int, default=1000)
    ap.add_argument("--many", type=int, default=4000)
    ap.add_argument("--max-det", type=int, default=100)
    ap.add_argument("--iou", type=float, default=0.5)
    ap.add_argument("--sigma", type=float, default=0.5)
    args = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    from multitask_hydranet_amd import HydraNet
    from multitask_hydranet_amd._lib import lib
    from multitask_hydranet_amd.postprocess import NMS_KINDS

    assert torch.cuda.is_available(), "needs the MI355X"
    dev = torch.device("cuda:0")
    cfgs = yaml.safe_load(open(os.path.join(ROOT, "cfgs", "hydranet_big.yml")))
    n, h, w = 16, 512, 1024
    k = cfgs["detection"]["num_classes"]
    anc = HydraNet(cfgs).anchors_for(h, w, dev).reshape(-1, 4).float().contiguous()
    a = anc.shape[0]
    gen = torch.Generator().manual_seed(0)
    cls = torch.sigmoid(torch.randn((n, a, k), generator=gen) * 1.5 - 4.0)
    reg = (torch.randn((n, a, 4), generator=gen) * 0.2).to(dev)
    best = np.sort(cls.max(dim=2)[0].numpy(), axis=1)
    cls = cls.to(dev)
    cap = 8192
    P = lambda t: t.data_ptr()
    rois = torch.empty((n, cap, 4), device=dev)
    cids = torch.empty((n, cap), device=dev, dtype=torch.int64)
    scores = torch.empty((n, cap), device=dev)
    kept = torch.empty((n,), device=dev, dtype=torch.int32)
    total = torch.empty((n,), device=dev, dtype=torch.int32)
    ws = {kind: torch.empty((lib().query("hn_det_post_ws_bytes_ex", n, cap, kind),), device=dev, dtype=torch.uint8) for kind in range(4)}
    res = {"anchors": a, "images": n, "classes": k, "cap": cap, "iou_threshold": args.iou, "sigma": args.sigma}
    runs = {}
    for label, want in (("few", args.few), ("many", args.many)):
        thr = float(np.median(best[:, -want]))                            # about `want` anchors of every image score above it
        head = lambda kind, thr=thr: (P(anc), P(reg), P(cls), n, a, k, h, w, thr, args.iou, cap, P(ws[kind]), P(rois), P(cids), P(scores), P(kept), P(total))
        runs[f"{label}_old_entry"] = (lambda head=head: lib().call("hn_det_postprocess", *head(0)))
        for kind, name in enumerate(NMS_KINDS):
            for max_det in (0, args.max_det):
                runs[f"{label}_{name}_max_det_{max_det}"] = (lambda head=head, kind=kind, max_det=max_det, thr=thr: lib().call(
                    "hn_det_postprocess_ex", *head(kind), kind, args.sigma, thr, max_det, 0))
        for name, fn in runs.items():
            if name.startswith(label):
                fn()
                torch.cuda.synchronize()
                assert int(total.max()) <= cap
                res[name + "_kept_per_image"] = float(kept.sum()) / n
        res[label + "_threshold"] = thr
        res[label + "_candidates_per_image"] = float(total.sum()) / n
        print(f"{label}: threshold {thr:.4f}, {res[label + '_candidates_per_image']:.0f} candidates per image", flush=True)
    ms = {name: [] for name in runs}
    for r in range(args.rounds):
        for name, fn in runs.items():
            ms[name].append(timed(fn, args.warmup, args.iters))
    for name in runs:
        res[name + "_us"] = 1e3 * statistics.median(ms[name])
        print(f"{name}: {res[name + '_us']:.1f} us, {res[name + '_kept_per_image']:.0f} kept per image (median of {args.rounds} rounds: "
              f"{', '.join('%.1f' % (1e3 * v) for v in ms[name])})", flush=True)
    print(json.dumps({k_: round(v, 3) if isinstance(v, float) else v for k_, v in res.items()}))


if __name__ == "__main__":
    main()
