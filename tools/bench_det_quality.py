"""Detection loss, forward + backward, for each detection.loss_cls_type (focal, qfl, vfl) under each IoU detection.loss_reg_type (giou,
diou, ciou) at the big cfg's detection shape (N = 16, the cfg's anchors at 512 x 1024, its K classes, Mx = 16 annotation rows of which
12 are boxes), timed with HIP events after warm-up.  The C entry points are called directly (hn_det_loss_iou_fwd/bwd for focal,
hn_det_loss_quality_fwd/bwd for qfl / vfl), two launches forward and one backward each.  Inputs as tools/bench_det_iou.py: the boxes are
perturbed copies of random anchors, so a realistic handful of anchors per box is positive; the positive rate and the positives' mean IoU
are printed.  The nine combinations are timed in alternating rounds of one process; the median over the rounds is reported.
Prints one line per measurement and a final JSON line."""
import argparse
import json
import os
import statistics
import sys

import torch
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KINDS = {"giou": 1, "diou": 2, "ciou": 3}
CLS_KINDS = {"focal": 0, "qfl": 1, "vfl": 2}


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
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    from multitask_hydranet_amd import HydraNet
    from multitask_hydranet_amd._lib import lib

    assert torch.cuda.is_available(), "needs the MI355X"
    dev = torch.device("cuda:0")
    cfgs = yaml.safe_load(open(os.path.join(ROOT, "cfgs", "hydranet_big.yml")))
    n, h, w, mx, boxes = 16, 512, 1024, 16, 12
    k = cfgs["detection"]["num_classes"]
    anc = HydraNet(cfgs).anchors_for(h, w, dev).reshape(-1, 4).float().contiguous()
    a = anc.shape[0]
    gen = torch.Generator().manual_seed(0)
    ac = anc.cpu()
    inside = ((ac[:, 0] >= 0) & (ac[:, 1] >= 0) & (ac[:, 2] <= h) & (ac[:, 3] <= w)).nonzero().flatten()
    ann = torch.full((n, mx, 5), -1.0)
    for i in range(n):
        pick = inside[torch.randperm(inside.numel(), generator=gen)[:boxes]]
        y1, x1, y2, x2 = ac[pick].unbind(1)
        d = (torch.rand(4, boxes, generator=gen) - 0.5) * 0.2
        ann[i, :boxes] = torch.stack([x1 + d[0] * (x2 - x1), y1 + d[1] * (y2 - y1), x2 + d[2] * (x2 - x1), y2 + d[3] * (y2 - y1),
                                      torch.randint(0, k, (boxes,), generator=gen).float()], dim=1)
    ann = ann.to(dev)
    cls = (torch.rand((n, a, k), generator=gen) * 0.2 + 0.01).to(dev)
    reg = (torch.randn((n, a, 4), generator=gen) * 0.2).to(dev)
    blocks = lib().query("hn_det_loss_blocks", a)
    assign = torch.empty((n, a), device=dev, dtype=torch.int16)
    part = torch.empty((n, blocks, 4), device=dev)
    npos = torch.empty((n,), device=dev)
    out = torch.empty((3,), device=dev)
    gout = torch.ones((2,), device=dev)
    dcls, dreg = torch.empty_like(cls), torch.empty_like(reg)
    P = lambda t: t.data_ptr()

    def step(kind, cls_kind):
        head = (P(cls), P(reg), P(anc), P(ann), n, a, k, mx, kind)
        if cls_kind == 0:
            lib().call("hn_det_loss_iou_fwd", *head, P(assign), P(part), P(npos), P(out))
            lib().call("hn_det_loss_iou_bwd", *head, P(assign), P(npos), P(gout), P(dcls), P(dreg))
        else:
            lib().call("hn_det_loss_quality_fwd", *head, cls_kind, None, 0, P(assign), P(part), P(npos), P(out))
            lib().call("hn_det_loss_quality_bwd", *head, cls_kind, None, P(assign), P(npos), P(gout), P(dcls), P(dreg))

    step(1, 1)
    torch.cuda.synchronize()
    rate = float(npos.sum()) / (n * a)
    print(f"N={n} A={a} K={k} Mx={mx}: {float(npos.sum()) / n:.1f} positives per image ({100 * rate:.3f} % of the anchors), "
          f"mean IoU of the positives {float(out[2]):.3f}", flush=True)
    combos = [(rn, cn) for rn in KINDS for cn in CLS_KINDS]
    ms = {c: [] for c in combos}
    for r in range(args.rounds):
        for rn, cn in combos:
            ms[(rn, cn)].append(timed(lambda: step(KINDS[rn], CLS_KINDS[cn]), args.warmup, args.iters))
    res = {"anchors": a, "positives_per_image": float(npos.sum()) / n}
    for rn, cn in combos:
        key = f"{cn}_{rn}_fwd_bwd_us"
        res[key] = 1e3 * statistics.median(ms[(rn, cn)])
        print(f"{cn} + {rn}: fwd + bwd {res[key]:.1f} us (median of {args.rounds} rounds: "
              f"{', '.join('%.1f' % (1e3 * v) for v in ms[(rn, cn)])})", flush=True)
    print(json.dumps({k_: round(v, 3) for k_, v in res.items()}))


if __name__ == "__main__":
    main()
