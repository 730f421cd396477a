"""What the weight average costs (optim.Adam(ema_decay=): hn_adam_step_ema in place of hn_adam_step / hn_adam_step_guarded -- one more read
and one more write per element inside the one Adam launch) and what the alternative would cost (torch._foreach_lerp_ over the same
tensors after the step).

optimizer.step() on the big cfg's parameter set with random gradients (no forward), HIP events around each step, median of --steps
(>= 50) after a warm-up:
  plain / plain + average            hn_adam_step        against hn_adam_step_ema
  guarded / guarded + average        hn_grad_guard + hn_adam_step_guarded against hn_grad_guard + hn_adam_step_ema with the record
  foreach_lerp                       torch._foreach_lerp_(averages, parameters, 1 - decay) alone
  swap                               optimizer.swap_ema() (hn_swap_many over every averaged parameter) alone

One JSON line."""
import argparse
import json
import os
import statistics
import sys

import torch
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as g  # noqa: E402

g.build()
from multitask_hydranet_amd import HydraNet  # noqa: E402
from multitask_hydranet_amd.optim import Adam  # noqa: E402


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


def main(steps, warmup, decay):
    dev = torch.device("cuda:0")
    cfgs = yaml.safe_load(open(os.path.join(ROOT, "cfgs", "hydranet_big.yml")))
    params = [p for p in HydraNet(cfgs).to(dev).parameters() if p.requires_grad]
    gen = torch.Generator(device=dev).manual_seed(0)
    for p in params:
        p.grad = torch.randn(p.shape, generator=gen, device=dev) * 1e-2
    out = dict(what="optimizer.step, big cfg parameter set", tensors=len(params), elements=sum(p.numel() for p in params), steps=steps,
               ema_decay=decay)
    guard = dict(max_grad_norm=1.0, skip_nonfinite=True)
    for name, kw in (("plain", {}), ("plain_ema", dict(ema_decay=decay)), ("guarded", guard), ("guarded_ema", dict(ema_decay=decay, **guard))):
        opt = Adam(params, 1e-5, **kw)
        out[name + "_ms"] = round(event_median(opt.step, steps, warmup), 4)
        if name == "plain_ema":
            out["averaged_tensors"] = len(opt.ema_named(enumerate(params)))
            out["swap_ms"] = round(event_median(opt.swap_ema, steps - steps % 2, warmup - warmup % 2), 4)      # an even count: live values back
        del opt
        torch.cuda.empty_cache()
    avgs = [p.detach().clone() for p in params]
    live = [p.detach() for p in params]
    out["foreach_lerp_ms"] = round(event_median(lambda: torch._foreach_lerp_(avgs, live, 1.0 - decay), steps, warmup), 4)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--decay", type=float, default=0.9998)
    a = ap.parse_args()
    if a.steps < 50:
        ap.error("--steps: medians are taken over at least 50 steps")
    main(a.steps, a.warmup, a.decay)
