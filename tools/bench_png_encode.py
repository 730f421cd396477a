"""PNG label encode on the device against PIL on one host core (png_encode.py): 16 class maps of 512 x 1024 written as
1080 x 1920 label PNGs -- 14 label-like maps (large constant regions with ragged boundaries, seeded) and the two 1080 x 1920 polygon
labels of tests/png_cases.py, decimated to 512 x 1024 --
  (a) device: png_encode.encode_streams (the launch sequence alone, between HIP events) and png_encode.encode_batch (end to end: launches,
      the one pinned copy back, the file framing on the host; wall clock), from an int64 mask that is already on the device;
  (b) host: the masks copied to the host, numpy nearest resize, Image.save(PNG) with PIL's defaults and with compress_level=1 (wall clock,
      one core).
--huffman fixed | dynamic | both picks the deflate code of (a); with both, the two are measured one after the other and the comparisons
with PIL speak of the dynamic one.  After a warm-up of each; medians of --repeats.  Every device file is decoded by PIL and compared with the host's resized map.  The device
time of the kernels one by one is left to a kernel trace (rocprofv3 --kernel-trace --stats).  Prints one line per measurement and a final
JSON line."""
import argparse
import io
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def label_like(h, w, seed, classes=5):
    g = np.random.Generator(np.random.Philox(seed))
    m = np.zeros((h, w), np.int64)
    for k in range(1, classes):
        edge = np.cumsum(g.integers(-2, 3, size=h)) + g.integers(w // 8, w - w // 8)
        m[np.arange(w)[None, :] > edge[:, None]] = k
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--src", type=int, nargs=2, default=[512, 1024])
    ap.add_argument("--out", type=int, nargs=2, default=[1080, 1920])
    ap.add_argument("--huffman", choices=("fixed", "dynamic", "both"), default="fixed", help="the deflate code of the device path; both: the "
                    "two one after the other in the same run")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_png_encode.py measures the MI355X"
    import __graft_entry__ as g
    g.build()
    from PIL import Image
    from multitask_hydranet_amd import png_encode
    from tests import png_cases

    hs, ws = args.src
    out_hw = tuple(args.out)
    maps = [label_like(hs, ws, 100 + k) for k in range(max(0, args.images - 2))]
    for data in png_cases.big_files()[:args.images - len(maps)]:
        big = png_cases.expected(data).astype(np.int64)
        maps.append(png_encode.resize_nearest(big, (hs, ws)))
    mask = torch.from_numpy(np.stack(maps)).cuda()
    n = len(maps)
    result = dict(images=n, src=[hs, ws], out=list(out_hw), chunk_bytes=png_encode.chunk_bytes())

    def device(huffman, key):
        files = png_encode.encode_batch(mask, out_sizes=out_hw, huffman=huffman)    # warm-up (code objects, allocator, pinned buffer)
        torch.cuda.synchronize()
        ev, wall = [], []
        for _ in range(args.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            st = png_encode.encode_streams(mask, out_sizes=out_hw, lean=True, huffman=huffman)
            e1.record()
            e1.synchronize()
            ev.append(e0.elapsed_time(e1))
            del st
            t0 = time.perf_counter()
            files = png_encode.encode_batch(mask, out_sizes=out_hw, huffman=huffman)
            wall.append(time.perf_counter() - t0)
        st = png_encode.encode_streams(mask, out_sizes=out_hw, lean=True, huffman=huffman)
        rec = st["buf"][:n * png_encode.RESULT_DTYPE.itemsize].cpu().numpy().view(png_encode.RESULT_DTYPE)
        result[key + "_status"] = [int(v) for v in rec["status"]]
        assert not any(result[key + "_status"]), "an image left the device path: the times below would be the host fallback's"
        result[key + "_stream_bytes"] = int(rec["stream_bytes"].sum())
        result[key + "_launches_event_ms"] = float(np.median(ev))
        result[key + "_end_to_end_wall_ms"] = 1e3 * float(np.median(wall))
        result[key + "_bytes"] = int(sum(len(f) for f in files))
        print("%-9s: %8.2f ms launch sequence (HIP events), %8.2f ms end to end with the copy back and the framing (wall), %d bytes"
              % (key.replace("device_", "dev "), result[key + "_launches_event_ms"], result[key + "_end_to_end_wall_ms"], result[key + "_bytes"]))
        return files

    # the fixed code keeps the keys it always had; the dynamic code's carry "dynamic"
    runs = {"fixed": ["fixed"], "dynamic": ["dynamic"], "both": ["fixed", "dynamic"]}[args.huffman]
    files = None
    for huffman in runs:
        files = device(huffman, "device" if huffman == "fixed" else "device_dynamic")
    key = "device" if runs[-1] == "fixed" else "device_dynamic"          # what the comparisons below speak of: the last one measured
    result["huffman"] = runs

    def host(**kw):
        t0 = time.perf_counter()
        arr = mask.cpu().numpy()
        blobs = []
        for k in range(n):
            bio = io.BytesIO()
            Image.fromarray(png_encode.resize_nearest(arr[k], out_hw).astype(np.uint8)).save(bio, "PNG", **kw)
            blobs.append(bio.getvalue())
        return time.perf_counter() - t0, blobs

    for name, kw in (("pil_default", {}), ("pil_level1", {"compress_level": 1})):
        host(**kw)
        runs = [host(**kw) for _ in range(max(1, args.repeats // 2))]
        ms = 1e3 * float(np.median([r[0] for r in runs]))
        nbytes = int(sum(len(b) for b in runs[0][1]))
        result[name + "_wall_ms"], result[name + "_bytes"] = ms, nbytes
        print("%-9s: %8.2f ms wall on one core (copy to the host, numpy resize, Image.save), %d bytes" % (name, ms, nbytes))

    same = True
    arr = mask.cpu().numpy()
    for k, f in enumerate(files):
        with Image.open(io.BytesIO(f)) as im:
            same = same and np.array_equal(np.asarray(im), png_encode.resize_nearest(arr[k], out_hw).astype(np.uint8))
    result.update(files_decode_to_the_maps=bool(same), wall_speedup_vs_pil_default=result["pil_default_wall_ms"] / result[key + "_end_to_end_wall_ms"],
                  size_vs_pil_default=result[key + "_bytes"] / result["pil_default_bytes"])
    if len(runs) == 2:
        result["dynamic_size_vs_fixed"] = result["device_dynamic_bytes"] / result["device_bytes"]
    print("device files decode to the resized maps: %s" % same)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
