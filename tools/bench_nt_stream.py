"""Per-shape A/B of the large-map 1x1 GEMM: hn_conv_gemm_nt (64 x 64 tile) against hn_conv_gemm_nt_stream, on the shapes of the training step.

Each arm is a captured graph of 20 launches (a ring of 4 input / output buffer sets, so that a launch does not find its own operands
in L2 any more than in the step), timed by HIP events; the figure is the median of 10 replays divided by 20, the spread is the
(max - min) / median of those replays.  GB/s on algorithmic bytes: x read once, out written once, weights once.

    python tools/bench_nt_stream.py [--wg K]        (K = wg_limit of the streaming arm, 0 = its default grid)
Prints a markdown table (profiles/nt_stream.md)."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multitask_hydranet_amd import ops as K      # noqa: E402

BF16, F32 = torch.bfloat16, torch.float32
SHAPES = [(174592, 112, 112), (131072, 112, 112), (32768, 112, 112), (8192, 112, 112), (2048, 112, 112), (131072, 112, 72)]
LAUNCHES, REPLAYS, RING = 20, 10, 4


def arm(stream, m, c0, nout, stats, wg):
    dev = torch.device("cuda:0")
    kp = K.kp32(c0)
    g = torch.Generator(device=dev)
    g.manual_seed(m + nout)
    xs = [torch.randn((m, c0), generator=g, device=dev).to(BF16) for _ in range(RING)]
    outs = [torch.empty((m, nout), device=dev, dtype=BF16) for _ in range(RING)]
    wp = K.pack_conv_weight((torch.randn((nout, c0, 1, 1), generator=g, device=dev) * 0.1).contiguous())[0]
    pr = K.lib().query("hn_nt_stat_rows", m, nout)
    ps = [torch.empty((pr, nout), device=dev, dtype=F32) for _ in range(RING)] if stats else [None] * RING
    pq = [torch.empty((pr, nout), device=dev, dtype=F32) for _ in range(RING)] if stats else [None] * RING

    def launch(i):
        x, o, a, b = xs[i % RING], outs[i % RING], ps[i % RING], pq[i % RING]
        if stream:
            K.lib().call("hn_conv_gemm_nt_stream", x.data_ptr(), c0, m, c0, K.ptr(wp), nout, kp, None, 0, o.data_ptr(), nout, K.ptr(a), K.ptr(b), wg)
        else:
            K.lib().call("hn_conv_gemm_nt", x.data_ptr(), None, 0, 0, 0, 0, c0, 0, c0, 0, 0, m, K.ptr(wp), nout, kp, 1, None, 0, o.data_ptr(), 0,
                         nout, 0, 0, K.ptr(a), K.ptr(b))

    launch(0)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for i in range(LAUNCHES):
            launch(i)
    graph.replay()
    torch.cuda.synchronize()
    times = []
    for _ in range(REPLAYS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        graph.replay()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) * 1000.0 / LAUNCHES)
    times.sort()
    med = 0.5 * (times[REPLAYS // 2 - 1] + times[REPLAYS // 2])
    return med, (times[-1] - times[0]) / med, (outs[0], ps[0], pq[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--wg", type=int, default=0)
    a = ap.parse_args()
    print("| rows | K -> N | stats | tile us | spread | GB/s | stream us | spread | GB/s | stream / tile | equal bits |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")
    for (m, c0, nout) in SHAPES:
        for stats in (False, True):
            t0, s0, r0 = arm(False, m, c0, nout, stats, 0)
            t1, s1, r1 = arm(True, m, c0, nout, stats, a.wg)
            same = all(x is None or bool((x.view(torch.int16 if x.dtype == BF16 else torch.int32) ==
                                          y.view(torch.int16 if y.dtype == BF16 else torch.int32)).all()) for x, y in zip(r0, r1))
            nbytes = 2.0 * m * (c0 + nout) + 2.0 * nout * K.kp32(c0)
            print("| %d | %d -> %d | %s | %.2f | %.1f %% | %.0f | %.2f | %.1f %% | %.0f | %.3f | %s |" %
                  (m, c0, nout, "yes" if stats else "no", t0, 100 * s0, nbytes / t0 / 1e3, t1, 100 * s1, nbytes / t1 / 1e3, t1 / t0,
                   "yes" if same else "NO"), flush=True)


if __name__ == "__main__":
    main()
