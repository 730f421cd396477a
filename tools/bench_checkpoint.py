"""What a full-state checkpoint costs (HydraTrainer.save_state / load_state; checkpoint.StatePacker, hn_ckpt.hip), next to torch.save /
torch.load of the module's and the optimizer's state_dict() -- the path a user has without it -- written to the same directory.

The big cfg's trainer with every option that adds state on (grad_clip_norm, skip_nonfinite, ema_decay, protect_bn_stats, ema_buffers),
one optimizer step on random gradients (no forward) so that moments, averages, the record and the keeper exist:
  pack_launch_ms        hn_state_pack alone on the cached tables (two launches: blocks, then the per-job fold): HIP events, median of --steps
  pack_tb_per_s         the HBM traffic rate that implies (one read and one write per word)
  save_async_stall_ms   what save_state(wait=False) puts on the training stream: HIP events around the call (the pack launch)
  save_async_call_ms    host time of that call (tables cached; the manifest's host-side state is collected here)
  save_async_closed_ms  host time from the call until checkpoint_wait() returns: the file is written, synced and renamed
  save_sync_ms          save_state(wait=True)
  load_state_ms         load_state: read, host-to-device copy, verify, unpack, the verdict's read, the host-side state
  torch_save_ms         torch.save({"model": net.state_dict(), "optim": optimizer.state_dict()})
  torch_load_ms         torch.load + both load_state_dict()
Host times are medians of --repeats.  One JSON line."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import torch
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as g  # noqa: E402

g.build()
from multitask_hydranet_amd._lib import lib  # noqa: E402
from multitask_hydranet_amd.train import HydraTrainer  # noqa: E402


def wall(fn, repeats):
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out)


def main(steps, repeats, where):
    cfgs = yaml.safe_load(open(os.path.join(ROOT, "cfgs", "hydranet_big.yml")))
    cfgs["train"].update(dict(continue_train=False, weight_file="", grad_clip_norm=10.0, skip_nonfinite=True, ema_decay=0.9998,
                              protect_bn_stats=True, ema_buffers=True))
    tr = HydraTrainer(cfgs, trainloader=None, validloader=None, iters_per_epoch=1000)
    gen = torch.Generator(device=tr.device).manual_seed(0)
    for p in tr.hydranet.parameters():
        p.grad = torch.randn(p.shape, generator=gen, device=tr.device) * 1e-2
    keeper = tr._keeper()
    keeper.snapshot()
    tr.optimizer.step()
    keeper.settle(tr.optimizer.guard_record)
    tr.scheduler.step()
    path, pth = os.path.join(where, "bench_state.hn"), os.path.join(where, "bench_state.pth")
    tr.save_state(path)                                             # builds the packer and its tables
    pk = tr._packer
    out = dict(what="full-state checkpoint of the big cfg's trainer", tensors=len(pk.named), words=pk.blob_words, mbytes=round(pk.blob_words * 4 / 1e6, 1),
               blocks=pk.blocks, steps=steps, repeats=repeats, file_bytes=os.path.getsize(path))
    _, jobs, _, owner = pk._plan()
    sums = pk.staging.data_ptr() + 4 * pk.blob_words

    def pack():
        lib().call("hn_state_pack", jobs.data_ptr(), owner.data_ptr(), pk.blocks, len(pk.named), pk._ws.data_ptr(), sums)
    for _ in range(5):
        pack()
    torch.cuda.synchronize()
    pairs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    for a, b in pairs:
        a.record()
        pack()
        b.record()
    torch.cuda.synchronize()
    ms = statistics.median(a.elapsed_time(b) for a, b in pairs)
    out["pack_launch_ms"] = round(ms, 4)
    out["pack_tb_per_s"] = round(2 * 4.0 * pk.blob_words / (ms * 1e-3) / 1e12, 3)
    stall, call, closed = [], [], []
    for _ in range(repeats):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        tr.save_state(path, wait=False)
        b.record()
        t1 = time.perf_counter()
        tr.checkpoint_wait()
        t2 = time.perf_counter()
        torch.cuda.synchronize()
        stall.append(a.elapsed_time(b))
        call.append((t1 - t0) * 1e3)
        closed.append((t2 - t0) * 1e3)
    out["save_async_stall_ms"] = round(statistics.median(stall), 3)
    out["save_async_call_ms"] = round(statistics.median(call), 2)
    out["save_async_closed_ms"] = round(statistics.median(closed), 1)
    out["save_sync_ms"] = round(wall(lambda: tr.save_state(path), repeats), 1)
    out["load_state_ms"] = round(wall(lambda: tr.load_state(path), repeats), 1)
    net, opt = tr.hydranet, tr.optimizer
    out["torch_save_ms"] = round(wall(lambda: torch.save({"model": net.state_dict(), "optim": opt.state_dict()}, pth), repeats), 1)
    out["torch_file_bytes"] = os.path.getsize(pth)

    def torch_load():
        sd = torch.load(pth, map_location=tr.device)
        net.load_state_dict(sd["model"])
        opt.load_state_dict(sd["optim"])
    out["torch_load_ms"] = round(wall(torch_load, repeats), 1)
    for f in (path, pth):
        os.remove(f)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--dir", default=tempfile.gettempdir(), help="where both files are written (the same filesystem for both)")
    a = ap.parse_args()
    if a.steps < 50:
        ap.error("--steps: medians are taken over at least 50 launches")
    main(a.steps, a.repeats, a.dir)
