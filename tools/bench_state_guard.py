"""What keeping the BatchNorm statistics in step with the guard and the weight average costs (bn_state.BufferKeeper: hn_state_guard twice
per step), next to optimizer.step() of the same trainer configuration.

The big cfg's persistent buffers (running_mean, running_var, num_batches_tracked of every BatchNorm) and its parameter set with random
gradients (no forward), HIP events around each call, median of --steps (>= 50) after a warm-up:
  snapshot            keeper.snapshot()                        hn_state_guard mode 0
  settle_protect      keeper.settle(record), shadows only      hn_state_guard mode 1 (the record says "not skipped": nothing is written)
  settle_average      keeper.settle(record), with averages     hn_state_guard mode 2
  snapshot_settle     both launches of a step, with averages
  optimizer_step      optim.Adam(max_grad_norm, skip_nonfinite, ema_decay).step(): hn_grad_guard + hn_adam_step_ema
  swap                keeper.swap() (hn_swap_many over the buffers) alone
  *_launch_us         hn_state_guard alone, 50 launches back to back on the cached tables (no per-call pointer check on the host)

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
from multitask_hydranet_amd.bn_state import BufferKeeper  # noqa: E402
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
    net = HydraNet(cfgs).to(dev)
    params = [p for p in net.parameters() if p.requires_grad]
    gen = torch.Generator(device=dev).manual_seed(0)
    for p in params:
        p.grad = torch.randn(p.shape, generator=gen, device=dev) * 1e-2
    opt = Adam(params, 1e-5, max_grad_norm=1.0, skip_nonfinite=True, ema_decay=decay)
    opt.step()                                                                     # (the record exists and says "not skipped")
    rec = opt.guard_record
    protect = BufferKeeper(net.named_buffers(), True)
    both = BufferKeeper(net.named_buffers(), True, ema_decay=decay)
    _, _, _, blocks, _, _ = both._plan()
    out = dict(what="BufferKeeper on the big cfg's BatchNorm buffers", tensors=len(both.live), words=sum(both.words), blocks=blocks, steps=steps,
               ema_decay=decay)

    def step_pair():
        both.snapshot()
        both.settle(rec)
    for name, fn in (("snapshot", both.snapshot), ("settle_protect", lambda: protect.settle(rec)), ("settle_average", lambda: both.settle(rec)),
                     ("snapshot_settle", step_pair), ("optimizer_step", opt.step)):
        out[name + "_ms"] = round(event_median(fn, steps, warmup), 4)
    # the launches alone: 50 back to back on the cached tables, without the keeper's per-call pointer check on the host
    from multitask_hydranet_amd._lib import lib
    _, jobs, owner, blk, _, _ = both._plan()
    for name, mode in (("snapshot", 0), ("settle_average", 2)):
        def burst(mode=mode):
            for _ in range(50):
                lib().call("hn_state_guard", jobs.data_ptr(), owner.data_ptr(), blk, mode, rec.data_ptr(), decay)
        out[name + "_launch_us"] = round(event_median(burst, max(steps // 5, 10), 2) * 1000.0 / 50, 2)
    out["swap_ms"] = round(event_median(both.swap, steps - steps % 2, warmup - warmup % 2), 4)        # an even count: live values back
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
