"""The demo's image output path: what the device half of the JPEG encode and the draw launch cost against their HBM
floors, what the host entropy stage costs against PIL's whole encode, and what the demo delivers end to end on image files.

    python tools/bench_demo_io.py [--n 16] [--iters 20] [--cfg cfgs/hydranet_big.yml] [--frames 12] [--no-demo]

Frame sets: 16 copies of the committed 2560x1440 sample frame (tests/golden/jpeg) and 16 synthetic 1920x1080 frames (smooth gradients +
noise, as tools/bench_jpeg.py).  Per set, at quality 95 / 4:2:0:
  encode kernel   hn_jpeg_encode over the batch by HIP events: mean of --iters launches after 3 warm-up runs, median and min..max of 5 such
                  windows, beside the HBM floor of the bytes it must move at 8 TB/s (frame in at 3 B/px, coefficients out at 2 B/sample)
  draw launch     hn_draw over the batch with a realistic list per frame (4 lanes of 40 points with their score text, 20 labelled boxes),
                  same windows; its floor is not stated: it reads no frame and writes only the painted pixels
  huffman stage   hn_jpeg_huff_encode (six launches) over the batch's coefficients, same windows, beside the HBM floor of reading the
                  coefficients once and writing the streams once; the pinned D2H copy of result records + scans at the capacity the scans
                  need (and at jpeg_encode's first-guess capacity) against the pageable copy of the coefficients; encode_batch end to end
                  per frame on frames already on the device, entropy="device" against entropy="host", alternated
  host, one core  hn_jpeg_entropy_encode per frame against PIL's Image.save of the same frame at the same settings (the only encoder a user
                  has without this path), and the D2H copy of the coefficients
  demo            frames per second over --frames files of the set, after 2 warm-up frames: Demo.process_device on
                  jpeg.imread_bgr_device (decode -> ... -> JPEG bytes, the frame never on the host) with the Huffman stage on the host
                  ("device") and on the device ("device_huff") against PIL decode -> Demo.process -> PIL save of the blended frame
                  (which draws nothing)
One JSON line per set.
"""
import argparse
import io
import json
import os
import sys
import time

import numpy as np
import torch
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from multitask_hydranet_amd import draw, jpeg, jpeg_encode     # noqa: E402
from multitask_hydranet_amd._lib import lib                     # noqa: E402

HBM_BPS = 8e12
QUALITY, SUBSAMPLING = 95, "4:2:0"


def synthetic_1080p(n):
    out = []
    for i in range(n):
        rng = np.random.default_rng(i)
        y, x = np.mgrid[0:1080, 0:1920]
        a = np.stack([x * 255.0 / 1919, y * 255.0 / 1079, ((x + 2 * y) * 0.5) % 256], 2) + rng.normal(0.0, 12.0, (1080, 1920, 3))
        out.append(np.clip(a, 0, 255).astype(np.uint8))
    return out


def spread(v):
    v = sorted(v)
    return {"median": round(v[len(v) // 2], 4), "min": round(v[0], 4), "max": round(v[-1], 4)}


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
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


def realistic_primitives(h, w):
    lanes = [{"score": 0.9 + 0.02 * k, "points": [{"x": w * (0.2 + 0.2 * k) + (0.5 - 0.25 * k) * 0.3 * w * t / 39.0, "y": h - 1 - 0.55 * h * t / 39.0}
                                                  for t in range(40)]} for k in range(4)]
    rs = np.random.RandomState(0)
    x0, y0 = rs.uniform(0, 0.8 * w, 20), rs.uniform(0.2 * h, 0.8 * h, 20)
    pred = {"rois": np.stack([x0, y0, x0 + rs.uniform(40, 0.2 * w, 20), y0 + rs.uniform(40, 0.2 * h, 20)], 1), "class_ids": rs.randint(0, 9, 20),
            "scores": rs.uniform(0.4, 1.0, 20)}
    names = ["roadtext", "pedestrian", "guidearrow", "traffic", "obstacle", "vehicle_wheel", "roadsign", "vehicle", "vehicle_light"]
    return draw.lane_primitives(lanes, w, filter_vertical=False) + draw.box_primitives(pred, (h, w), names, (w, h), (w, h))


def device_times(frames, iters, dev):
    from multitask_hydranet_amd.augment import pack
    pk = pack(frames)
    pk = {"data": pk["data"].to(dev), "offsets": pk["offsets"], "shapes": pk["shapes"]}
    heads, desc, coff = jpeg_encode.describe_batch(pk["shapes"], pk["offsets"], QUALITY, SUBSAMPLING)
    desc_d = torch.from_numpy(desc.view(np.uint8).copy()).to(dev)
    coefs = torch.empty((int(coff[-1]) // 2,), device=dev, dtype=torch.int16)
    args = (pk["data"].data_ptr(), int(pk["data"].numel()), desc_d.data_ptr(), len(heads), max(h["mcus_y"] for h in heads),
            max(h["mcus_x"] * 8 * h["hs"] for h in heads), coefs.data_ptr(), int(coefs.numel()) * 2)
    enc = window(lambda: lib().call("hn_jpeg_encode", *args), iters)
    bgr_bytes, coef_bytes = int(sum(f.size for f in frames)), int(sum(h["coef_bytes"] for h in heads))
    floor = (bgr_bytes + coef_bytes) / HBM_BPS * 1e3
    d2h = window(lambda: coefs.cpu(), max(2, iters // 4))
    huff = huffman_times(pk, heads, coefs, coff, iters, dev)
    lists = [realistic_primitives(*f.shape[:2]) for f in frames]
    scratch = {"data": pk["data"].clone(), "offsets": pk["offsets"], "shapes": pk["shapes"]}
    t = time.perf_counter()
    draw.draw_packed(scratch, lists)
    torch.cuda.synchronize()
    first = (time.perf_counter() - t) * 1e3                              # with the host-side record building and the upload
    n = len(frames)
    imgs = np.zeros(n, dtype=draw.IMAGE_DTYPE)
    p = 0
    for i, e in enumerate(imgs):
        e["off"], e["W"], e["H"], e["p0"], e["p1"] = int(pk["offsets"][i]), frames[i].shape[1], frames[i].shape[0], p, p + len(lists[i])
        p += len(lists[i])
    blob = torch.from_numpy(np.concatenate([imgs.view(np.uint8), draw.to_records([q for l in lists for q in l]).view(np.uint8)])).to(dev)
    dargs = (scratch["data"].data_ptr(), int(scratch["data"].numel()), blob.data_ptr(), n, max(f.shape[0] for f in frames),
             max(f.shape[1] for f in frames), blob.data_ptr() + 24 * n, p)
    drw = window(lambda: lib().call("hn_draw", *dargs), iters)
    return {"frames": n, "bgr_MB": round(bgr_bytes / 1e6, 2), "coef_MB": round(coef_bytes / 1e6, 2), "encode_kernel_ms": spread(enc),
            "hbm_floor_ms": round(floor, 4), "achieved_over_floor": round(spread(enc)["median"] / floor, 2), "coef_d2h_ms": spread(d2h),
            "primitives_per_frame": len(lists[0]), "draw_launch_ms": spread(drw), "draw_call_with_host_side_ms": round(first, 3), "huffman": huff}


def huffman_times(pk, heads, coefs, coff, iters, dev):
    n = len(heads)
    blobs = jpeg_encode.entropy_encode_device(heads, coefs, coff)      # (the coefficients are in place: device_times ran the encode kernel)
    hdr = [len(jpeg_encode.write_header(h)) for h in heads]
    scans = [len(b) - x - 2 for b, x in zip(blobs, hdr)]
    out = {}
    for label, caps in (("exact", scans), ("first_guess", [jpeg_encode.first_capacity(h) for h in heads])):
        desc, ooff = jpeg_encode.huff_describe(heads, coff, caps)
        max_blocks, max_cap = max(h["coef_bytes"] // 128 for h in heads), max(caps)
        ws = torch.empty((jpeg_encode.huff_workspace_bytes(n, max_blocks, max_cap),), device=dev, dtype=torch.uint8)
        desc_d = torch.from_numpy(desc.view(np.uint8).copy()).to(dev)
        buf = torch.empty((16 * n + int(ooff[-1]),), device=dev, dtype=torch.uint8)
        args = (coefs.data_ptr(), int(coefs.numel()) * 2, desc_d.data_ptr(), n, max_blocks, max_cap, ws.data_ptr(), int(ws.numel()),
                buf.data_ptr() + 16 * n, int(ooff[-1]), buf.data_ptr())
        ms = window(lambda: lib().call("hn_jpeg_huff_encode", *args), iters)
        stage = torch.empty((int(buf.numel()),), dtype=torch.uint8, pin_memory=True)
        copy = window(lambda: stage.copy_(buf, non_blocking=True), max(2, iters // 4))
        status = stage[:16 * n].numpy().view(jpeg_encode.HUFF_RESULT_DTYPE)["status"]
        out[label] = {"capacity_MB": round(int(ooff[-1]) / 1e6, 2), "launches_ms": spread(ms), "workspace_MB": round(int(ws.numel()) / 1e6, 1),
                      "pinned_d2h_ms": spread(copy), "images_too_small": int((status == jpeg_encode.CAPACITY_TOO_SMALL).sum())}
    coef_bytes = int(sum(h["coef_bytes"] for h in heads))
    floor = (coef_bytes + sum(scans)) / HBM_BPS * 1e3
    out["stream_MB"] = round(sum(scans) / 1e6, 3)
    out["hbm_floor_ms"] = round(floor, 4)
    out["achieved_over_floor"] = round(out["exact"]["launches_ms"]["median"] / floor, 1)
    e2e = {"host": [], "device": []}
    for _ in range(3):                                                   # alternated; the first round is the warm-up
        for mode in ("host", "device"):
            torch.cuda.synchronize()
            t = time.perf_counter()
            got = jpeg_encode.encode_batch(pk, QUALITY, SUBSAMPLING, entropy=mode)
            e2e[mode].append((time.perf_counter() - t) * 1e3 / n)
            assert got == blobs
    out["encode_batch_ms_per_frame"] = {m: spread(v[1:]) for m, v in e2e.items()}
    return out


def pil_save(bgr):
    from PIL import Image
    bio = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(bgr[..., ::-1])).save(bio, "JPEG", quality=QUALITY, subsampling=SUBSAMPLING)
    return bio.getvalue()


def host_times(frames, dev):
    ent, pil, sizes = [], [], []
    for f in frames[:8]:
        heads, coefs, coff = jpeg_encode.encode_coefs_device([f], QUALITY, SUBSAMPLING)
        host = coefs.cpu().numpy()[:heads[0]["coef_bytes"] // 2]
        for _ in range(3):
            t = time.perf_counter()
            blob = jpeg_encode.entropy_encode(host, heads[0])
            ent.append((time.perf_counter() - t) * 1e3)
            t = time.perf_counter()
            ref = pil_save(f)
            pil.append((time.perf_counter() - t) * 1e3)
        sizes.append((len(blob), len(ref)))
    return {"entropy_stage_ms": spread(ent), "pil_save_ms": spread(pil), "pil_over_entropy": round(spread(pil)["median"] / spread(ent)["median"], 2),
            "stream_bytes_ours_vs_pil": [int(np.mean([s[0] for s in sizes])), int(np.mean([s[1] for s in sizes]))]}


def demo_rates(frames, cfg, count, dev):
    from multitask_hydranet_amd.demo import Demo
    torch.manual_seed(0)
    demo = Demo(yaml.safe_load(open(cfg)))
    demo.det_conf = 0.95                                                # random initialisation: see demo.main
    files = [pil_save(f) for f in frames[:4]]
    warm = 2
    res = {}
    for mode in ("device", "device_huff", "pil") * 2:                    # alternated: two windows per mode
        t0 = None
        for i in range(warm + count):
            if i == warm:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
            data = files[i % len(files)]
            if mode != "pil":
                out = demo.process_device(jpeg.imread_bgr_device(data, device=dev), QUALITY, SUBSAMPLING,
                                          entropy="device" if mode == "device_huff" else "host")["jpeg"]
            else:
                out = pil_save(demo.process(jpeg.pil_bgr(data))["visual"])
            assert len(out) > 1000
        torch.cuda.synchronize()
        res.setdefault("%s_frames_per_s" % mode, []).append(round(count / (time.perf_counter() - t0), 2))
    res["frames_timed"] = count
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=16)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--cfg", default=os.path.join(ROOT, "cfgs", "hydranet_big.yml"))
    ap.add_argument("--frames", type=int, default=12)
    ap.add_argument("--no-demo", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_demo_io.py measures on the GPU"
    dev = torch.device("cuda:0")
    sample = jpeg.pil_bgr(open(os.path.join(ROOT, "tests", "golden", "jpeg", "frame_2560x1440.jpg"), "rb").read())
    sets = {"synthetic_1920x1080": [np.ascontiguousarray(f[..., ::-1]) for f in synthetic_1080p(a.n)], "sample_2560x1440": [sample] * a.n}
    for name, frames in sets.items():
        res = {"set": name, "quality": QUALITY, "subsampling": SUBSAMPLING, "device": device_times(frames, a.iters, dev), "host": host_times(frames, dev)}
        if not a.no_demo:
            res["demo"] = demo_rates(frames, a.cfg, a.frames, dev)
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
