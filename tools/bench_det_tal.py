"""Task-aligned anchor assignment (detection.assigner = tal, hn_det_tal.hip) at the big cfg's detection shape, next to ATSS in the same
run: N = 16, the cfg's anchors at 512 x 1024 (A = 98 208), Mx = 16 annotation rows of which --boxes are boxes (log-uniform sides, uniform
centres, as tools/bench_det_atss.py), predictions from a seeded generator (scores sigmoid(N(-2.5, 1.5)), regression N(0, 0.25)), timed
with HIP events after warm-up.  The C entry points are called directly:
  (a) hn_det_tal_assign: its three launches (select, per-anchor assignment, normalise), and hn_det_atss_assign's three;
  (b) the VFL + GIoU loss forward + backward (two launches + one) that reads (a)'s outputs: hn_det_loss_aligned_fwd / _bwd on TAL's
      assignment and target, hn_det_loss_quality_fwd / _bwd on ATSS's assignment;
  (c) (a) + (b): the loss side of a step under either assigner, six launches each.
The measurements are timed in alternating rounds of one process; the median over the rounds is reported.  Also prints how many boxes end
without a positive anchor under either rule.  Prints one line per measurement and a final JSON line."""
import argparse
import ctypes
import json
import math
import os
import statistics
import sys

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
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--boxes", type=int, default=12)
    ap.add_argument("--topk", type=int, default=13)
    ap.add_argument("--atss-topk", type=int, default=9)
    args = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    from multitask_hydranet_amd import HydraNet
    from multitask_hydranet_amd._lib import lib

    assert torch.cuda.is_available(), "needs the MI355X"
    dev = torch.device("cuda:0")
    cfgs = yaml.safe_load(open(os.path.join(ROOT, "cfgs", "hydranet_big.yml")))
    n, h, w, mx, boxes = 16, 512, 1024, 16, args.boxes
    k = cfgs["detection"]["num_classes"]
    net = HydraNet(cfgs)
    anc = net.anchors_for(h, w, dev).reshape(-1, 4).float().contiguous()
    level_sizes, apl = net.anchor_level_sizes(h, w), net.anchors_per_location
    a = anc.shape[0]
    gen = torch.Generator().manual_seed(0)
    ann = torch.full((n, mx, 5), -1.0)
    side = torch.exp(torch.rand(n, boxes, 2, generator=gen) * (math.log(400.0) - math.log(8.0)) + math.log(8.0))
    cx, cy = torch.rand(n, boxes, generator=gen) * w, torch.rand(n, boxes, generator=gen) * h
    ann[:, :boxes, 0], ann[:, :boxes, 2] = (cx - side[..., 0] / 2).clamp(0, w - 1), (cx + side[..., 0] / 2).clamp(0, w - 1)
    ann[:, :boxes, 1], ann[:, :boxes, 3] = (cy - side[..., 1] / 2).clamp(0, h - 1), (cy + side[..., 1] / 2).clamp(0, h - 1)
    ann[:, :boxes, 4] = torch.randint(0, k, (n, boxes), generator=gen).float()
    ann = ann.to(dev)
    cls = torch.sigmoid(torch.randn((n, a, k), generator=gen) * 1.5 - 2.5).to(dev)
    reg = (torch.randn((n, a, 4), generator=gen) * 0.25).to(dev)
    blocks = lib().query("hn_det_loss_blocks", a)
    sizes = (ctypes.c_int * len(level_sizes))(*level_sizes)
    lv = (ctypes.addressof(sizes), len(level_sizes), args.atss_topk, apl)
    ws_atss = torch.empty((lib().query("hn_det_atss_ws_bytes", n, a, mx, *lv),), device=dev, dtype=torch.uint8)
    ws_tal = torch.empty((lib().query("hn_det_tal_ws_bytes", n, a, mx, args.topk),), device=dev, dtype=torch.uint8)
    assign_atss = torch.empty((n, a), device=dev, dtype=torch.int16)
    assign_tal = torch.empty((n, a), device=dev, dtype=torch.int16)
    target = torch.empty((n, a), device=dev)
    thr = torch.empty((n, mx), device=dev)
    part = torch.empty((n, blocks, 4), device=dev)
    npos = torch.empty((n,), device=dev)
    out = torch.empty((3,), device=dev)
    gout = torch.tensor([1.0, 50.0], device=dev)
    dcls, dreg = torch.empty_like(cls), torch.empty_like(reg)
    P = lambda t: t.data_ptr()
    head = (P(cls), P(reg), P(anc), P(ann), n, a, k, mx, 1, 2, None)                  # giou, vfl, no mask

    def atss():
        lib().call("hn_det_atss_assign", P(anc), P(ann), n, a, mx, *lv, P(ws_atss), P(assign_atss), P(thr))

    def tal():
        lib().call("hn_det_tal_assign", P(anc), P(reg), P(cls), P(ann), n, a, k, mx, args.topk, P(ws_tal), P(assign_tal), P(target))

    def loss_atss():
        lib().call("hn_det_loss_quality_fwd", *head, 1, P(assign_atss), P(part), P(npos), P(out))
        lib().call("hn_det_loss_quality_bwd", *head, P(assign_atss), P(npos), P(gout), P(dcls), P(dreg))

    def loss_tal():
        lib().call("hn_det_loss_aligned_fwd", *head, 1, P(assign_tal), P(target), P(part), P(npos), P(out))
        lib().call("hn_det_loss_aligned_bwd", *head, P(assign_tal), P(target), P(npos), P(gout), P(dcls), P(dreg))

    def step_atss():
        atss()
        loss_atss()

    def step_tal():
        tal()
        loss_tal()

    atss()
    tal()
    torch.cuda.synchronize()
    res = {"anchors": a, "images": n, "boxes_per_image": boxes, "tal_topk": args.topk, "atss_topk": args.atss_topk}
    for name, t in (("atss", assign_atss), ("tal", assign_tal)):
        hit = torch.zeros((n, mx), dtype=torch.bool, device=dev)
        for i in range(n):
            hit[i, t[i][t[i] >= 0].long().unique()] = True
        res[name + "_positives_per_image"] = float((t >= 0).sum()) / n
        res[name + "_boxes_without_positive"] = int(n * boxes - int(hit.sum()))
        print(f"{name}: {res[name + '_positives_per_image']:.1f} positives per image, {res[name + '_boxes_without_positive']} of {n * boxes} "
              "boxes without a positive anchor", flush=True)
    runs = {"tal_assign_3_launches": tal, "atss_assign_3_launches": atss, "loss_fwd_bwd_on_tal_3_launches": loss_tal,
            "loss_fwd_bwd_on_atss_3_launches": loss_atss, "tal_plus_loss_6_launches": step_tal, "atss_plus_loss_6_launches": step_atss}
    ms = {name: [] for name in runs}
    for r in range(args.rounds):
        for name, fn in runs.items():
            ms[name].append(timed(fn, args.warmup, args.iters))
    for name in runs:
        res[name + "_us"] = 1e3 * statistics.median(ms[name])
        print(f"{name}: {res[name + '_us']:.1f} us (median of {args.rounds} rounds: {', '.join('%.1f' % (1e3 * v) for v in ms[name])})", flush=True)
    print(json.dumps({k_: round(v, 3) if isinstance(v, float) else v for k_, v in res.items()}))


if __name__ == "__main__":
    main()
