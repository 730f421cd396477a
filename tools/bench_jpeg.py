"""JPEG decode split: what the host entropy stage costs against PIL's full decode, what the device stage costs against
its HBM floor, what the scan decode on the device costs, and what a DataLoader -> HydraTrainer.to_gpu pipeline delivers with decode="host",
decode="device" and decode="device-entropy".

    python tools/bench_jpeg.py [--files DIR] [--set NAME] [--scan-only] [--n 16] [--iters 20] [--workers 8] [--batches 96] [--out-hw 512x1024]

Frame sets: the committed 2560x1440 sample frame (tests/golden/jpeg) and, as tools/bench_augment.py, synthetic 1920x1080 frames (smooth
gradients + noise, quality 90, 4:2:0); --files DIR adds every *.jpg of a directory as a third set.  Per set, on ONE core (this process):
PIL's full decode and the entropy stage (parse + Huffman) per frame, median and min..max over the set x 3 passes.  Then for --n frames of
the set: the pinned H2D copy of the packed coefficients and the two device kernels by HIP events (mean of --iters after 3 warm-up runs,
min..max of 5 such windows), beside the HBM floor of the bytes they must move at 8 TB/s; the same for the files' bytes and the scan decode
(hn_jpeg_scan_decode: two memsets + three launches; --scan-only runs just that, for a kernel trace).  Then the loader: DataLoader(num_workers=k,
pin_memory) over a data list of the set (its files listed over and over; lane + box labels; no label maps, so the decode is what
differs) -> to_gpu, images per second over --batches batches after 4 warm-up batches, for the three decode modes at the same k, two windows
each, alternated.  The window is longer than the loader's prefetch depth (2 k batches), so it measures production, not a drained queue,
and the data list ends with the window, so every loader runs to its natural end.
"""
import argparse
import glob
import io
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from multitask_hydranet_amd import jpeg                         # noqa: E402
from multitask_hydranet_amd._lib import lib                     # noqa: E402
from multitask_hydranet_amd.dataset import MultitaskData        # noqa: E402

HBM_BPS = 8e12


def synthetic_1080p(n):
    from PIL import Image
    out = []
    for i in range(n):
        rng = np.random.default_rng(i)
        y, x = np.mgrid[0:1080, 0:1920]
        a = np.stack([x * 255.0 / 1919, y * 255.0 / 1079, ((x + 2 * y) * 0.5) % 256], 2) + rng.normal(0.0, 12.0, (1080, 1920, 3))
        bio = io.BytesIO()
        Image.fromarray(np.clip(a, 0, 255).astype(np.uint8)).save(bio, "JPEG", quality=90, subsampling="4:2:0")
        out.append(bio.getvalue())
    return out


def spread(v):
    v = sorted(v)
    return {"median": round(v[len(v) // 2], 3), "min": round(v[0], 3), "max": round(v[-1], 3)}


def host_times(streams):
    pil, ent = [], []
    for _ in range(3):
        for s in streams:
            t = time.perf_counter()
            jpeg.pil_bgr(s)
            pil.append((time.perf_counter() - t) * 1e3)
            t = time.perf_counter()
            head = jpeg.parse(s)
            jpeg.entropy_decode(s, head)
            ent.append((time.perf_counter() - t) * 1e3)
    return {"pil_full_decode_ms": spread(pil), "entropy_stage_ms": spread(ent),
            "pil_frames_per_s_per_core": round(1e3 / spread(pil)["median"], 1), "entropy_frames_per_s_per_core": round(1e3 / spread(ent)["median"], 1)}


def scan_times(streams, n, iters, dev, window):
    """the upload of the files' bytes and hn_jpeg_scan_decode on --n frames; the coefficients are checked against the host's once"""
    items = [jpeg.stream_stage(streams[i % len(streams)]) for i in range(n)]
    pk = jpeg.pack_streams(items, pin=True)
    ent = jpeg.entropy_decode_device(pk, device=dev)
    assert int(ent["status"].abs().sum()) == 0
    want = jpeg.entropy_decode(streams[0], items[0][0]).reshape(-1)
    assert np.array_equal(ent["data"][:want.size].cpu().numpy(), want), "device coefficients differ from the host's"
    h2d = window(lambda: pk["data"].to(dev, non_blocking=True))
    scans = pk["scans"]
    data, desc = pk["data"].to(dev), torch.from_numpy(scans.view(np.uint8).copy()).to(dev)
    max_scan, max_blocks = int(scans["scan_bytes"].max()), max(jpeg.n_blocks(it[0]) for it in items)
    wsb = int(lib().query("hn_jpeg_scan_ws_bytes", n, max_scan, max_blocks))
    ws = torch.empty((wsb,), device=dev, dtype=torch.uint8)
    coefs = torch.empty((pk["coef_bytes"] // 2,), device=dev, dtype=torch.int16)
    status = torch.zeros((n,), device=dev, dtype=torch.int32)
    ker = window(lambda: lib().call("hn_jpeg_scan_decode", data.data_ptr(), int(data.numel()), desc.data_ptr(), n, max_scan, max_blocks,
                                    ws.data_ptr(), wsb, coefs.data_ptr(), int(coefs.numel()) * 2, status.data_ptr()))
    return {"stream_MB": round(int(pk["data"].numel()) / 1e6, 2), "scan_MB": round(int(scans["scan_bytes"].sum()) / 1e6, 2),
            "h2d_pinned_ms": spread(h2d), "scan_decode_ms": spread(ker)}


def device_times(streams, n, iters, dev, scan_only=False):
    items = [jpeg.host_stage(streams[i % len(streams)]) for i in range(n)]
    assert all(h is not None for h, _ in items), "the set holds a JPEG outside the supported set"
    pk = jpeg.pack_coefs(items, pin=True)
    desc, idx, offs, shapes, plane_total = jpeg.describe_batch(pk)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def window(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(5):
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1) / iters)
        return ms
    if scan_only:
        return {"frames": n, "scan": scan_times(streams, n, iters, dev, window)}
    h2d = window(lambda: pk["data"].to(dev, non_blocking=True))
    coefs = pk["data"].to(dev)
    desc_d = torch.from_numpy(desc.view(np.uint8).copy()).to(dev)
    planes = torch.empty((plane_total,), device=dev, dtype=torch.uint8)
    dst = torch.empty((int(offs[-1]),), device=dev, dtype=torch.uint8)
    args = (coefs.data_ptr(), int(coefs.numel()) * 2, desc_d.data_ptr(), n, max(jpeg.n_blocks(h) for h, _ in items), int(shapes[:, 0].max()),
            int(shapes[:, 1].max()), planes.data_ptr(), plane_total, dst.data_ptr(), int(dst.numel()))
    ker = window(lambda: lib().call("hn_jpeg_decode", *args))
    coef_bytes = sum(h["coef_bytes"] for h, _ in items)
    moved = coef_bytes + 2 * plane_total + int(offs[-1])              # coefficients in, planes out and in again, BGR out
    floor = moved / HBM_BPS * 1e3
    return {"frames": n, "coef_MB": round(coef_bytes / 1e6, 2), "bgr_MB": round(int(offs[-1]) / 1e6, 2), "planes_MB": round(plane_total / 1e6, 2),
            "h2d_pinned_ms": spread(h2d), "h2d_GBps": round(pk["data"].numel() * 2 / (spread(h2d)["median"] * 1e-3) / 1e9, 1),
            "kernels_ms": spread(ker), "hbm_floor_ms": round(floor, 4), "achieved_over_floor": round(spread(ker)["median"] / floor, 2),
            "scan": scan_times(streams, n, iters, dev, window)}


WARM = 4


def loader_rates(streams, n_files, workers, batch, batches, out_hw, dev):
    from multitask_hydranet_amd.train import HydraTrainer
    import yaml
    root = tempfile.mkdtemp(prefix="bench_jpeg_")
    try:
        for sub in ("images", "labels_lane", "labels_object"):
            os.makedirs(os.path.join(root, sub))
        paths = []
        for i in range(min(n_files, len(streams), 16)):
            p = os.path.join(root, "images", "f%04d.jpg" % i)
            open(p, "wb").write(streams[i % len(streams)])
            head = jpeg.parse(streams[i % len(streams)])
            w, h = head["width"], head["height"]
            json.dump({"shapes": [{"label": "l", "points": [[0.3 * w + k, h - 1.0 - 0.04 * h * k] for k in range(20)]}] * 4},
                      open(p.replace(".jpg", ".json").replace("images", "labels_lane"), "w"))
            open(p.replace(".jpg", ".txt").replace("images", "labels_object"), "w").write("100,100,300,260,2\n" * 12)
            paths.append(p)
        open(os.path.join(root, "train.txt"), "w").write("\n".join(paths[i % len(paths)] for i in range(n_files)) + "\n")
        cfgs = yaml.safe_load(open(os.path.join(ROOT, "cfgs", "hydranet_tiny.yml")))
        cfgs["dataloader"].update(data_list=root, network_input_height=out_hw[0], network_input_width=out_hw[1], with_aug=True)
        cfgs["train"].update(train_seg=False)
        tr = HydraTrainer(cfgs, iters_per_epoch=10)
        res = {}
        for mode in ("host", "device", "device-entropy") * 2:               # alternated: two windows per mode
            ds = MultitaskData(cfgs, "train", decode=mode)
            loader = torch.utils.data.DataLoader(ds, batch_size=batch, shuffle=False, num_workers=workers, collate_fn=ds.collate_fn, pin_memory=True,
                                                 drop_last=True)
            seen, t0 = 0, None
            for b in loader:
                out = tr.to_gpu(b)
                torch.cuda.synchronize()
                seen += 1
                if seen == WARM:
                    t0 = time.perf_counter()
            assert seen == WARM + batches, "the data list and the timed window differ"
            res.setdefault("%s_img_per_s" % mode, []).append(round(batches * batch / (time.perf_counter() - t0), 1))
            del loader
        res["workers"], res["batch"], res["batches"] = workers, batch, batches
        return res
    finally:
        shutil.rmtree(root, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", default=None)
    ap.add_argument("--n", type=int, default=16)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--workers", type=int, default=8)
    ap.add_argument("--batches", type=int, default=96)
    ap.add_argument("--out-hw", default="512x1024")
    ap.add_argument("--no-loader", action="store_true")
    ap.add_argument("--set", default=None, help="measure only the frame set of this name")
    ap.add_argument("--scan-only", action="store_true", help="only the scan decode's upload and kernels (for a kernel trace)")
    a = ap.parse_args()
    assert 0 < a.workers <= 16
    out_hw = tuple(int(v) for v in a.out_hw.split("x"))
    assert torch.cuda.is_available(), "bench_jpeg.py measures on the GPU"
    dev = torch.device("cuda:0")
    sets = {"sample_2560x1440": [open(os.path.join(ROOT, "tests", "golden", "jpeg", "frame_2560x1440.jpg"), "rb").read()],
            "synthetic_1920x1080": synthetic_1080p(8)}
    if a.files:
        sets["files"] = [open(p, "rb").read() for p in sorted(glob.glob(os.path.join(a.files, "*.jpg")))]
    for name, streams in sets.items():
        if a.set and name != a.set:
            continue
        if a.scan_only:
            print(json.dumps({"set": name, "device": device_times(streams, a.n, a.iters, dev, scan_only=True)}), flush=True)
            continue
        res = {"set": name, "files": len(streams), "host": host_times(streams), "device": device_times(streams, a.n, a.iters, dev)}
        if not a.no_loader:
            res["loader"] = loader_rates(streams, a.n * (a.batches + WARM), a.workers, a.n, a.batches, out_hw, dev)
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
