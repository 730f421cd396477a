"""What gradient accumulation costs per micro-batch (optim.GradAccumulator: one hn_grad_accum launch), next to optimizer.step() with and
without grads= on the same trainer configuration.

The big cfg's parameter set with random gradients (no forward), HIP events around each call, median of --steps (>= 50) after a warm-up:
  add_first           accumulator.add() as micro-batch 1 (acc = g: one read, one write per element), host-side table check included
  add_next            accumulator.add() as micro-batch 2 (acc += (g - acc) / 2: two reads, one write per element)
  *_launch_us         hn_grad_accum alone, 20 launches back to back on the cached tables, and the HBM traffic rate that implies
  optimizer_step      optim.Adam(max_grad_norm, skip_nonfinite, ema_decay).step(): hn_grad_guard + hn_adam_step_ema on p.grad
  optimizer_step_acc  the same step(grads=accumulator, guard_words=[sticky word]): the same kernels on the accumulator's views

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
from multitask_hydranet_amd.optim import Adam, GradAccumulator  # noqa: E402


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
    loss = torch.ones((), device=dev)
    word = torch.zeros((1,), dtype=torch.int32, device=dev)
    acc = GradAccumulator(params)
    opt = Adam(params, 1e-5, max_grad_norm=1.0, skip_nonfinite=True, ema_decay=decay)
    numel = sum(p.numel() for p in params)

    def add_first():
        acc.reset()
        acc.add(losses=[loss], guard_words=[word])

    def add_next():
        acc.pending = 1
        acc.add(losses=[loss], guard_words=[word])
    add_first()
    _, jobs, owner, blocks = acc._table
    out = dict(what="GradAccumulator on the big cfg's parameters", tensors=len(params), elements=numel, blocks=blocks, steps=steps, ema_decay=decay)
    out["add_first_ms"] = round(event_median(add_first, steps, warmup), 4)
    out["add_next_ms"] = round(event_median(add_next, steps, warmup), 4)
    # the launches alone: 20 back to back on the cached tables, without the accumulator's per-call gradient check on the host
    from multitask_hydranet_amd._lib import lib
    for name, j, passes in (("add_first", 1, 2), ("add_next", 2, 3)):
        def burst(j=j):
            for _ in range(20):
                lib().call("hn_grad_accum", jobs.data_ptr(), owner.data_ptr(), blocks, j, None, 0, None, None, 0, acc.sticky_word.data_ptr())
        us = event_median(burst, max(steps // 5, 10), 2) * 1000.0 / 20
        out[name + "_launch_us"] = round(us, 2)
        out[name + "_tb_per_s"] = round(passes * 4.0 * numel / (us * 1e-6) / 1e12, 3)
    out["optimizer_step_ms"] = round(event_median(lambda: opt.step(losses=[loss], guard_words=[word]), steps, warmup), 4)
    add_first()
    out["optimizer_step_acc_ms"] = round(event_median(lambda: opt.step(grads=acc, losses=[loss], guard_words=[word, acc.sticky_word]), steps, warmup), 4)
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
