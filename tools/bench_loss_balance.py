"""The total loss under train.loss_balance: uncertainty against the static weights, forward + backward through the ops layer
(ops.balanced_loss_sum -> hn_balanced_sum; ops.weighted_loss_sum -> hn_weighted_sum) on the six loss scalars of a joint step in their
three groups, and what stepping the log-variances adds to a step: hn_balance_hold, the one-tensor optim.Adam (its hn_grad_guard with
skip_nonfinite), hn_balance_hold.  Two figures each: the eager call (autograd nodes, allocations and launches from the host: what an
uncaptured step pays; the optimizer's launches are always issued eagerly) and the same launches captured in a hipGraph and replayed
(the kernels alone).  Timed with HIP events after warm-up in alternating rounds of one process; the median over the rounds is
reported.  Prints one line per measurement and a final JSON line."""
import argparse
import json
import os
import statistics
import sys

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--iters", type=int, default=500)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    from multitask_hydranet_amd import ops as K
    from multitask_hydranet_amd._lib import lib
    from multitask_hydranet_amd.optim import Adam

    assert torch.cuda.is_available(), "needs the MI355X"
    dev = torch.device("cuda:0")
    xs = [torch.tensor(v, device=dev, requires_grad=True) for v in (8.5, 59.0, 0.22, 4.9, 9.7, 0.92)]
    groups = lambda: [(1.0, [(xs[0], 1.0)]), (1.0, [(xs[1], 1.0), (xs[2], 50.0)]), (1.0, [(xs[3], 1.0), (xs[4], 1.0), (xs[5], 5.0)])]
    s = torch.zeros(6, device=dev)
    s._hn_mut_cell = [0]
    ga = torch.zeros(12, device=dev)
    rec = torch.zeros(16, device=dev)
    one = torch.ones((), device=dev)
    sums = {"weighted": lambda: K.weighted_loss_sum(groups()), "balanced": lambda: K.balanced_loss_sum(groups(), s, ga, 6.0, record=rec)}

    def eager(name):
        def step():
            for x in xs:
                x.grad = None
            sums[name]().backward(one)
        return step

    def captured(name):
        step = eager(name)
        st = torch.cuda.Stream()
        st.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(st):
            for _ in range(3):
                step()
        torch.cuda.current_stream().wait_stream(st)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        for x in xs:
            x.grad = None
        with torch.cuda.graph(graph):
            sums[name]().backward(one)
        return graph.replay

    steps = {(name, how): make(name) for name in sums for how, make in (("eager", eager), ("graph", captured))}

    # the log-variances' step, as HydraTrainer._balance_step issues it
    def adam_step(guarded):
        s.grad = ga[:6]
        opt = Adam([s], 1e-3, weight_decay=0.0, skip_nonfinite=guarded)
        opt.state[s] = dict(step=torch.zeros((), dtype=torch.float32), exp_avg=torch.zeros_like(s), exp_avg_sq=torch.zeros_like(s))
        hold = torch.zeros(18, device=dev)
        word = torch.zeros(1, dtype=torch.int32, device=dev)
        st = opt.state[s]
        t = (s.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), hold.data_ptr())

        def step():
            lib().call("hn_balance_hold", *t, None, 6)
            opt.step(**(dict(guard_words=[word]) if guarded else {}))
            lib().call("hn_balance_hold", *t, ga[6:].data_ptr(), 6)
        return step
    steps[("log_var_step", "eager")] = adam_step(False)
    steps[("log_var_step_guarded", "eager")] = adam_step(True)

    ms = {k: [] for k in steps}
    for r in range(args.rounds):
        for k, fn in steps.items():
            ms[k].append(timed(fn, args.warmup, args.iters))
    res = {}
    for (name, how), v in ms.items():
        key = f"{name}_{how}_us"
        res[key] = round(1e3 * statistics.median(v), 2)
        print(f"{name} ({how}): {res[key]:.2f} us (median of {args.rounds} rounds: {', '.join('%.2f' % (1e3 * x) for x in v)})", flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
