"""Lovasz-softmax seg loss (segment.use_lovasz) on the bench workload (N=16, 3 x 512 x 1024 images -> 16 x 5 x 512 x 1024 seg logits),
timed with HIP events after warm-up:
  (a) hn_seg_lovasz_fwd + hn_seg_lovasz_bwd_s2d on seeded logits / targets (also each alone, and the fp32-dlogits backward);
  (b) the torch-ROCm restatement a reference user would run (softmax + torch.sort + cumsum per class, autograd backward), same tensors;
  (c) the captured big-cfg training step (HydraTrainer(capture_step=True), as tools/trainer_bench.py) with use_lovasz off and on.
Prints one line per measurement and a final JSON line.  --skip-step leaves (c) out (e.g. under a kernel tracer)."""
import argparse
import json
import os
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


def torch_lovasz(probas, labels, ignore=255):
    """the reference's computation restated in torch ops (fp32, unstable sort), on [N, C, H, W] probabilities"""
    c = probas.shape[1]
    p = probas.permute(0, 2, 3, 1).reshape(-1, c)
    lab = labels.reshape(-1)
    keep = lab != ignore
    p, lab = p[keep], lab[keep]
    losses = []
    for k in range(c):
        fg = (lab == k).float()
        if fg.sum() == 0:
            continue
        e = (fg - p[:, k]).abs()
        es, perm = torch.sort(e, 0, descending=True)
        fs = fg[perm]
        gts = fs.sum()
        jac = 1.0 - (gts - fs.cumsum(0)) / (gts + (1.0 - fs).cumsum(0))
        jac[1:] = jac[1:] - jac[:-1]
        losses.append(torch.dot(es, jac))
    return torch.stack(losses).mean()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--skip-step", action="store_true")
    args = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    from multitask_hydranet_amd._lib import lib
    from multitask_hydranet_amd import ops as K

    dev = torch.device("cuda:0")
    n, h, w, c = 16, 512, 1024, 5
    gen = torch.Generator(device=dev).manual_seed(0)
    logits = torch.randn((n, h, w, c), device=dev, generator=gen) * 2.0
    target = torch.randint(0, c, (n, h, w), device=dev, generator=gen).to(torch.float32)
    target[:, : h // 8] = 255.0
    hw = h * w
    res = {}
    ws = torch.empty((lib().query("hn_seg_lovasz_ws_bytes", n, hw, c),), device=dev, dtype=torch.uint8)
    out = torch.empty((1,), device=dev)
    gout = torch.ones((1,), device=dev)
    dz = K.new_act(n, h // 2, w // 2, K.pad8(4 * c), dev)
    dl = torch.empty_like(logits)
    P = lambda t: t.data_ptr()
    fwd = lambda: lib().call("hn_seg_lovasz_fwd", P(logits), c, c, P(target), 1, 255, n, hw, P(ws), P(out))
    s2d = lambda: lib().call("hn_seg_lovasz_bwd_s2d", P(logits), c, c, P(target), 1, 255, n, h, w, P(ws), P(gout), P(dz), K.ld(dz))
    bwd = lambda: lib().call("hn_seg_lovasz_bwd", P(logits), c, c, P(target), 1, 255, n, hw, P(ws), P(gout), P(dl), c)
    res["hip_fwd_bwd_s2d_ms"] = timed(lambda: (fwd(), s2d()), args.warmup, args.iters)
    res["hip_fwd_ms"] = timed(fwd, args.warmup, args.iters)
    res["hip_bwd_s2d_ms"] = timed(s2d, args.warmup, args.iters)
    res["hip_bwd_fp32_ms"] = timed(bwd, args.warmup, args.iters)
    res["workspace_mb"] = ws.numel() / 1e6
    for k, v in res.items():
        print(f"(a) {k}: {v:.3f}", flush=True)

    x = logits.permute(0, 3, 1, 2).detach().requires_grad_(True)
    lab = target.long()

    def ref_step():
        x.grad = None
        torch_lovasz(torch.softmax(x, 1), lab).backward()

    res["torch_sort_fwd_bwd_ms"] = timed(ref_step, 2, max(3, args.iters // 4))
    print(f"(b) torch restatement fwd + bwd: {res['torch_sort_fwd_bwd_ms']:.3f} ms", flush=True)
    del x, dl, ws
    torch.cuda.empty_cache()

    if not args.skip_step:
        from bench import synthetic_batch
        from multitask_hydranet_amd.train import HydraTrainer
        cfgs = yaml.safe_load(open(os.path.join(ROOT, "cfgs", "hydranet_big.yml")))
        cfgs["dataloader"]["network_input_height"], cfgs["dataloader"]["network_input_width"] = h, w
        cfgs["train"].update(dict(continue_train=False, weight_file="", epoch=1, lr=1e-4, weight_decay=0.0))
        batch = synthetic_batch(cfgs, n, h, w, seed=1, device=dev)
        for lovasz in (False, True):
            cfgs["segment"]["use_lovasz"] = lovasz
            torch.manual_seed(0)
            tr = HydraTrainer(cfgs, trainloader=None, validloader=None, iters_per_epoch=1000, capture_step=True)
            tr.hydranet.check_finite = False
            tr.hydranet.lane_points_per_line = h // cfgs["lane"]["interval"]
            ms = timed(lambda: tr.train_step(dict(batch)), args.warmup, args.iters)
            key = "step_lovasz_ms" if lovasz else "step_ce_ms"
            res[key] = ms
            print(f"(c) captured big-cfg step, use_lovasz={lovasz}: {ms:.3f} ms ({n / ms * 1e3:.1f} img/s)", flush=True)
            del tr
            torch.cuda.empty_cache()
        res["step_delta_ms"] = res["step_lovasz_ms"] - res["step_ce_ms"]
    print(json.dumps({k: round(v, 4) for k, v in res.items()}))


if __name__ == "__main__":
    main()
