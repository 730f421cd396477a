"""Every loss under a per-image task mask (gt_dict["task_valid"]) against its unmasked twin, forward + backward through the ops
layer (ops/losses.py: the autograd node and its launches, as cal_loss issues them), at N = 16 and the big cfg's shapes: seg logits
16 x 512 x 1024 x 5, the cfg's anchors at 512 x 1024 with its K classes and 12 boxes per image, 8 192 lane rows of 322 columns.  The mask
has every second image unlabelled.  Timed with HIP events after warm-up; masked and unmasked alternate in rounds of one process and the
median over the rounds is reported.  Prints one line per loss and a final JSON line."""
import argparse
import json
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
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    from multitask_hydranet_amd import HydraNet, ops as K

    assert torch.cuda.is_available(), "needs the MI355X"
    dev = torch.device("cuda:0")
    cfgs = yaml.safe_load(open(os.path.join(ROOT, "cfgs", "hydranet_big.yml")))
    n, h, w, c = 16, 512, 1024, 5
    gen = torch.Generator().manual_seed(0)
    valid = torch.tensor([1, 0] * (n // 2), dtype=torch.uint8, device=dev)

    seg = (torch.randn((n, h, w, c), generator=gen) * 2).to(dev).permute(0, 3, 1, 2).requires_grad_(True)
    tgt = torch.randint(0, c, (n, h, w), generator=gen).float()
    tgt[:, : h // 8] = 255
    tgt = tgt.to(dev)
    cw = torch.tensor(cfgs["segment"]["class_weight"], dtype=torch.float32, device=dev)
    ratio = cfgs["segment"]["top_k_ratio"]

    kc, mx, boxes = cfgs["detection"]["num_classes"], 16, 12
    anc = HydraNet(cfgs).anchors_for(h, w, dev).reshape(-1, 4).float().contiguous()
    ac = anc.cpu()
    inside = ((ac[:, 0] >= 0) & (ac[:, 1] >= 0) & (ac[:, 2] <= h) & (ac[:, 3] <= w)).nonzero().flatten()
    ann = torch.full((n, mx, 5), -1.0)
    for i in range(n):
        pick = inside[torch.randperm(inside.numel(), generator=gen)[:boxes]]
        y1, x1, y2, x2 = ac[pick].unbind(1)
        d = (torch.rand(4, boxes, generator=gen) - 0.5) * 0.2
        ann[i, :boxes] = torch.stack([x1 + d[0] * (x2 - x1), y1 + d[1] * (y2 - y1), x2 + d[2] * (x2 - x1), y2 + d[3] * (y2 - y1),
                                      torch.randint(0, kc, (boxes,), generator=gen).float()], dim=1)
    ann = ann.to(dev)
    cls = (torch.rand((n, anc.shape[0], kc), generator=gen) * 0.2 + 0.01).to(dev).requires_grad_(True)
    reg = (torch.randn((n, anc.shape[0], 4), generator=gen) * 0.2).to(dev).requires_grad_(True)

    rows, L, wcol = 512, 322, 160
    lz = (torch.randn((n, rows, 2), generator=gen) * 2).to(dev).requires_grad_(True)
    pos = torch.rand((n, rows), generator=gen) < 0.03
    lt = torch.stack([~pos, pos], -1).float().to(dev)
    loc_t = (torch.randint(-40, 41, (n, rows, L), generator=gen) / 8.0 * (torch.rand((n, rows, L), generator=gen) < 0.7)).to(dev)
    loc_p = (loc_t + torch.randn((n, rows, L), generator=gen).to(dev)).requires_grad_(True)

    def run(loss, leaves):
        torch.autograd.grad(loss, leaves)

    def lane(v):
        kw = {} if v is None else dict(valid=v, rows_per_image=rows)
        p, ng, pm, aux = K.lane_cls_loss_hip(lt, lz, **kw)
        return p + ng + K.lane_loc_loss_hip(pm, aux, loc_t, loc_p, points_per_line=wcol, **kw)

    def det(fn, v, **kw):
        out = fn(cls, reg, anc, ann, **kw, **({} if v is None else dict(valid=v)))
        return out[0].sum() + out[1].sum()

    cases = {
        "seg_topk": lambda v: run(K.seg_loss_hip(seg, tgt, cw, True, ratio, **({} if v is None else dict(valid=v))), (seg,)),
        "seg_focal": lambda v: run(K.seg_focal_loss_hip(seg, tgt.clamp(max=c - 1), cw, **({} if v is None else dict(valid=v))), (seg,)),
        "seg_lovasz": lambda v: run(K.seg_lovasz_loss_hip(seg, tgt, **({} if v is None else dict(valid=v))), (seg,)),
        "det_smooth_l1": lambda v: run(det(K.det_loss_hip, v), (cls, reg)),
        "det_ciou": lambda v: run(det(K.det_iou_loss_hip, v, kind="ciou"), (cls, reg)),
        "lane_cls_loc": lambda v: run(lane(v), (lz, loc_p)),
    }
    res = {}
    for name, fn in cases.items():
        ms = {"unmasked": [], "masked": []}
        for _ in range(args.rounds):
            ms["unmasked"].append(timed(lambda: fn(None), args.warmup, args.iters))
            ms["masked"].append(timed(lambda: fn(valid), args.warmup, args.iters))
        for key in ms:
            res[f"{name}_{key}_us"] = 1e3 * statistics.median(ms[key])
        print(f"{name}: fwd + bwd unmasked {res[name + '_unmasked_us']:.1f} us, masked (8 of 16 images labelled) {res[name + '_masked_us']:.1f} us "
              f"(rounds: {', '.join('%.1f / %.1f' % (1e3 * a, 1e3 * b) for a, b in zip(ms['unmasked'], ms['masked']))})", flush=True)
    print(json.dumps({k_: round(v, 1) for k_, v in res.items()}))


if __name__ == "__main__":
    main()
