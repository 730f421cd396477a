"""Device augmentation cost: 16 synthetic 1920x1080 frames under the reference's plan distribution -> 640x640 and 512x1024.
Reports the kernels' device-event time (photometric + warp/area/normalise + seg), the host time of collate (pack + plans + label
transforms, no decode), the pinned H2D copy of the packed frames and, for scale, PIL's JPEG decode of one frame.

    python tools/bench_augment.py [--iters 20] [--split]

--split: dataloader.do_split plans (split ratio 0.5; the photometric draws are those of the plain run) and the host cost of
augment.cal_split on one 4-lane label.
"""
import argparse
import io
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multitask_hydranet_amd import augment as A            # noqa: E402
from multitask_hydranet_amd._lib import lib                 # noqa: E402
from multitask_hydranet_amd.dataset import collate          # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--n", type=int, default=16)
    ap.add_argument("--split", action="store_true")
    a = ap.parse_args()
    ratio = 0.5 if a.split else None
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    H, W = 1080, 1920
    frames = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(a.n)]
    segs = [rng.integers(0, 8, (H, W), dtype=np.uint8) for _ in range(a.n)]
    boxes = [np.array([[100, 100, 300, 260, 1]] * 12, dtype=np.float64) for _ in range(a.n)]
    lanes = [{"Lines": [[{"x": 900.0 + 10 * k, "y": 1079.0 - 40 * k} for k in range(20)]] * 4, "Labels": ["l"] * 4} for _ in range(a.n)]
    res = {}
    # host collate (no decode): pack + plans
    items = [dict(src_frame=f, src_seg=s, det_raw=b, lane_raw=l, src_image_shape=dict(width=W, height=H, channel=3), src_image_path="", annot_lane_path="",
                  aug_plan=A.sample_plan(0, 0, i, do_split=a.split, split_ratio=ratio)) for i, (f, s, b, l) in enumerate(zip(frames, segs, boxes, lanes))]
    t = time.perf_counter()
    for _ in range(3):
        batch = collate(items, 640, 640)
    res["host_collate_ms"] = (time.perf_counter() - t) / 3 * 1e3
    pinned = batch["src_frames"]["data"].pin_memory()
    for _ in range(2):
        pinned.to(dev, non_blocking=True)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.iters):
        src = pinned.to(dev, non_blocking=True)
    e1.record()
    torch.cuda.synchronize()
    res["h2d_ms"] = e0.elapsed_time(e1) / a.iters
    res["h2d_GBps"] = pinned.numel() / (res["h2d_ms"] * 1e-3) / 1e9
    for out_hw in ((640, 640), (512, 1024)):
        plans = [A.sample_plan(0, 1, i, do_split=a.split, split_ratio=ratio) for i in range(a.n)]
        t = time.perf_counter()
        out = A.augment_batch(batch["src_frames"], lanes, boxes, batch["src_segs"], plans, out_hw, dev)   # labels + descriptors + launches
        torch.cuda.synchronize()
        res["augment_batch_first_call_ms_%dx%d" % out_hw[::-1]] = (time.perf_counter() - t) * 1e3
        # kernels alone on device-resident inputs
        desc = np.zeros(a.n, dtype=A.DESC_DTYPE)
        ws_total = 0
        for i, p in enumerate(plans):
            d = A.describe(p, W, H)
            e = desc[i]
            e["finv"], e["p"], e["op"], e["per_channel"], e["radius"], e["w"] = d["finv"], d["p"], d["op"], d["per_channel"], d["radius"], d["w"]
            e["seed_lo"], e["seed_hi"] = d["seed"] & 0xFFFFFFFF, d["seed"] >> 32 & 0xFFFFFFFF
            e["Hs"], e["Ws"], e["src_off"], e["seg_off"] = H, W, batch["src_frames"]["offsets"][i], batch["src_segs"]["offsets"][i]
            e["ws_off"] = ws_total if d["op"] else -1
            ws_total += H * W * 3 if d["op"] else 0
        desc_d = torch.from_numpy(desc.view(np.uint8).copy()).to(dev)
        seg_d = batch["src_segs"]["data"].to(dev)
        ws = torch.empty((max(1, ws_total),), device=dev, dtype=torch.uint8)
        img = torch.empty((a.n, 3) + out_hw, device=dev)
        gseg = torch.empty((a.n,) + out_hw, device=dev, dtype=torch.uint8)
        L = lib()

        def run():
            if ws_total:
                L.call("hn_augment_photometric", src.data_ptr(), desc_d.data_ptr(), a.n, H, W, ws.data_ptr())
            L.call("hn_augment_image", src.data_ptr(), ws.data_ptr(), desc_d.data_ptr(), a.n, out_hw[0], out_hw[1], img.data_ptr())
            L.call("hn_augment_seg", seg_d.data_ptr(), desc_d.data_ptr(), a.n, out_hw[0], out_hw[1], gseg.data_ptr())
        for _ in range(3):
            run()
        torch.cuda.synchronize()
        e0.record()
        for _ in range(a.iters):
            run()
        e1.record()
        torch.cuda.synchronize()
        res["kernels_ms_%dx%d" % out_hw[::-1]] = e0.elapsed_time(e1) / a.iters
        res["photometric_images_%dx%d" % out_hw[::-1]] = int((desc["op"] > 0).sum())
        res["split_crops_%dx%d" % out_hw[::-1]] = sum(p.get("split", {}).get("crop") is not None for p in plans)
    if a.split:
        # two lanes leaning in, two leaning out, 20 points each: one image's cal_split on this core
        split_lanes = {"Lines": [[{"x": x0 + dx * k, "y": 1079.0 - 25 * k} for k in range(20)]
                                 for x0, dx in ((300.0, 20.0), (700.0, 8.0), (1200.0, -8.0), (1700.0, -20.0))]}
        assert A.cal_split(split_lanes, W, H)[0]
        t = time.perf_counter()
        for _ in range(2000):
            A.cal_split(split_lanes, W, H)
        res["cal_split_us_per_item"] = (time.perf_counter() - t) / 2000 * 1e6
    from PIL import Image
    bio = io.BytesIO()
    Image.fromarray(frames[0]).save(bio, format="JPEG", quality=90)
    t = time.perf_counter()
    for _ in range(3):
        np.asarray(Image.open(io.BytesIO(bio.getvalue())).convert("RGB"))
    res["pil_decode_ms_per_frame"] = (time.perf_counter() - t) / 3 * 1e3
    print(json.dumps({k: round(v, 3) if isinstance(v, float) else v for k, v in res.items()}))


if __name__ == "__main__":
    main()
