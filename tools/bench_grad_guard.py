"""What the gradient guard costs (optim.Adam(max_grad_norm=, skip_nonfinite=): hn_grad_guard's three launches + hn_adam_step_guarded in
place of hn_adam_step) and what train.skip_nonfinite gives back (the host guard's synchronising reads of the losses).

1. optimizer.step() on the big cfg's parameter set with random gradients (no forward): guard off against guard on, HIP events around
   each step, median of --steps (>= 50) after a warm-up.
2. a captured tiny-cfg trainer step (one hipGraph replay + Adam + LR step) with and without train.skip_nonfinite: HIP events per step and
   wall time per step of a run that synchronises once at its end.

One JSON line per measurement."""
import argparse
import copy
import json
import os
import statistics
import sys
import time

import torch
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as g  # noqa: E402

g.build()
from multitask_hydranet_amd import HydraNet  # noqa: E402
from multitask_hydranet_amd.optim import Adam  # noqa: E402
from multitask_hydranet_amd.train import HydraTrainer  # noqa: E402
from tests.helpers import load_cfg, load_npz, tiny_state  # noqa: E402


def event_median(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    pairs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    for a, b in pairs:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return statistics.median(a.elapsed_time(b) for a, b in pairs)


def optimizer_step(steps, warmup):
    dev = torch.device("cuda:0")
    cfgs = yaml.safe_load(open(os.path.join(ROOT, "cfgs", "hydranet_big.yml")))
    params = [p for p in HydraNet(cfgs).to(dev).parameters() if p.requires_grad]
    gen = torch.Generator(device=dev).manual_seed(0)
    for p in params:
        p.grad = torch.randn(p.shape, generator=gen, device=dev) * 1e-2
    numel = sum(p.numel() for p in params)
    out = dict(what="optimizer.step, big cfg parameter set", tensors=len(params), elements=numel, steps=steps)
    for name, kw in (("off", {}), ("on", dict(max_grad_norm=1.0, skip_nonfinite=True))):
        opt = Adam(params, 1e-5, **kw)
        out[name + "_ms"] = round(event_median(opt.step, steps, warmup), 4)
        if kw:
            out["record"] = opt.grad_guard_record()
        del opt
        torch.cuda.empty_cache()
    print(json.dumps(out), flush=True)


def captured_trainer_step(steps, warmup):
    z = load_npz("tiny_hydranet.npz")
    cfgs = load_cfg("hydranet_tiny.yml")
    cfgs["train"].update(dict(continue_train=False, weight_file="", epoch=1, lr=1e-6, weight_decay=0.0))
    batch = {k[3:]: torch.from_numpy(z[k].copy()).cuda() for k in z.files if k.startswith("in/")}
    out = dict(what="captured tiny-cfg trainer step", steps=steps)
    for name, keys in (("host_guard", {}), ("skip_nonfinite", dict(skip_nonfinite=True))):
        c = copy.deepcopy(cfgs)
        c["train"].update(keys)
        tr = HydraTrainer(c, trainloader=None, validloader=None, iters_per_epoch=100000, capture_step=True)
        tr.hydranet.load_state_dict(tiny_state(z))
        tr.hydranet.lane_points_per_line = int(z["meta/lane_points_per_line"])
        fn = lambda: tr.train_step(dict(batch))
        out[name + "_event_ms"] = round(event_median(fn, steps, max(warmup, 4)), 4)
        assert tr._cap is not None
        walls = []
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                fn()
            torch.cuda.synchronize()
            walls.append((time.perf_counter() - t0) / steps * 1e3)
        out[name + "_wall_ms"] = round(statistics.median(walls), 4)
        if keys:
            out["record"] = tr.optimizer.grad_guard_record()
        del tr
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--only", choices=("optimizer", "trainer"), default=None)
    a = ap.parse_args()
    if a.steps < 50:
        ap.error("--steps: medians are taken over at least 50 steps")
    if a.only != "trainer":
        optimizer_step(a.steps, a.warmup)
    if a.only != "optimizer":
        captured_trainer_step(a.steps, a.warmup)
