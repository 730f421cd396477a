"""Lane location loss, forward + backward through the ops layer, for each lane.loss_loc_type at the workload's lane shape (N = 16 at
640 x 640: M = 16 * 400 anchor rows, P = 80 points per line, L = 162 columns), timed with HIP events after warm-up.  smooth_l1 is
ops.lane_loc_loss_hip, liou is ops.lane_liou_loss_hip (half width 15 px / interval 8), both on the pmask / aux that one
ops.lane_cls_loss_hip call left; two launches forward and one backward each.  About 4 % of the rows are positive, a row's valid points
are two contiguous runs next to the length columns, as the encoder writes them.  Two figures per type: the eager call (autograd nodes,
allocations and launches from the host: what an uncaptured step pays) and the same call captured in a hipGraph and replayed (the
kernels alone: what a captured step pays).  The types are timed in alternating rounds of one process; the median over the rounds is
reported.  Prints one line per measurement and a final JSON line."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

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


def inputs(n, rows, ppl, dev, seed=0):
    g = np.random.default_rng(seed)
    m, L = n * rows, 2 * ppl + 2
    pos = g.random(m) < 0.04
    t = np.zeros((m, L), np.float32)
    down, up = g.integers(0, ppl + 1, m), g.integers(0, ppl + 1, m)
    x = (g.integers(-40, 41, (m, L)) / 8.0 + 1.0 / 16.0).astype(np.float32)      # (no zero among the valid offsets)
    col = np.arange(ppl)
    t[:, :ppl] = np.where(col[None, :] < down[:, None], x[:, :ppl], 0.0)
    t[:, ppl + 2:] = np.where(col[None, :] < up[:, None], x[:, ppl + 2:], 0.0)
    t[:, ppl], t[:, ppl + 1] = down, up
    p = (t + g.standard_normal((m, L)) * 1.5).astype(np.float32)
    z = (g.standard_normal((m, 2)) * 2).astype(np.float32)
    ct = np.stack([~pos, pos], 1).astype(np.float32)
    f = lambda a, *shape: torch.from_numpy(a).to(dev).view(*shape)
    return f(z, n, rows, 2), f(ct, n, rows, 2), f(p, n, rows, L), f(t, n, rows, L), int(pos.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    from multitask_hydranet_amd import ops as K

    assert torch.cuda.is_available(), "needs the MI355X"
    dev = torch.device("cuda:0")
    n, rows, ppl, interval = 16, (640 // 32) ** 2, 640 // 8, 8
    z, ct, p, t, npos = inputs(n, rows, ppl, dev)
    with torch.no_grad():
        _, _, pmask, aux = K.lane_cls_loss_hip(ct, z)
    p.requires_grad_(True)
    e = 15.0 / interval
    losses = {"smooth_l1": lambda: K.lane_loc_loss_hip(pmask, aux, t, p, points_per_line=ppl),
              "liou": lambda: K.lane_liou_loss_hip(pmask, aux, t, p, e)[0]}

    def eager(name):
        def step():
            p.grad = None
            losses[name]().backward()
        return step

    def captured(name):
        step = eager(name)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(3):
                step()
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        p.grad = None
        with torch.cuda.graph(graph):
            losses[name]().backward()
        return graph.replay

    print(f"M={n * rows} L={2 * ppl + 2} P={ppl} e={e}: {npos} positive rows ({100.0 * npos / (n * rows):.2f} %)", flush=True)
    steps = {(name, how): make(name) for name in losses for how, make in (("eager", eager), ("graph", captured))}
    ms = {k: [] for k in steps}
    for r in range(args.rounds):
        for k, fn in steps.items():
            ms[k].append(timed(fn, args.warmup, args.iters))
    res = {"rows": n * rows, "columns": 2 * ppl + 2, "positive_rows": npos}
    for (name, how), v in ms.items():
        key = f"{name}_{how}_fwd_bwd_us"
        res[key] = 1e3 * statistics.median(v)
        print(f"{name} ({how}): fwd + bwd {res[key]:.1f} us (median of {args.rounds} rounds: {', '.join('%.1f' % (1e3 * x) for x in v)})", flush=True)
    print(json.dumps({k_: round(v, 3) if isinstance(v, float) else v for k_, v in res.items()}))


if __name__ == "__main__":
    main()
