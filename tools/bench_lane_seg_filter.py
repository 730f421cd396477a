"""The lane filter by the seg head's marking class on the device against numpy on one host core (lane_codec.LaneSegFilter,
hn_lane_filter.hip): 16 images of 640 x 640 (400 anchors of 80 points), 14 selected lanes each, a label-like class map.
  (a) device: hn_lane_seg_filter's launch sequence alone, between HIP events, on the decode's device arrays;
  (b) lane_codec.decode_batch end to end (launches, the readback, the Lane objects; wall clock) without and with the filter;
  (c) host: the class maps copied to the host (the 3.3 MB per frame the filter saves) and the same counts in numpy on one core, every
      segment painted inside its own bounding box (wall clock); its counts must equal the device's;
  (d) --demo: Demo.process_device_batch on the big cfg with random weights, 8 frames of 720p, the switch off and on (wall clock per group).
      With --demo-only the file runs in a checkout that has no filter yet (the switch is then never passed): the same figure at the parent.
After a warm-up of each; medians of --repeats.  Prints one line per measurement and a final JSON line."""
import argparse
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


def head_outputs(n, lanes, codec, seed=3):
    """logits whose decode leaves `lanes` lanes per image: bottom-row anchors, full height, leaning by a seeded amount"""
    g = np.random.Generator(np.random.Philox(seed))
    fw, hw, ppl = codec.feature_width, codec.feature_size, codec.points_per_line
    assert lanes <= fw
    cls = np.zeros((n, hw, 2), np.float32)
    cls[:, :, 0] = 6.0
    loc = np.zeros((n, hw, 2 * ppl + 2), np.float32)
    for i in range(n):
        for k, w in enumerate(sorted(g.choice(fw, lanes, replace=False).tolist())):
            a = hw - fw + w
            cls[i, a] = (0.0, 3.0 + 0.1 * k)
            loc[i, a, ppl + 1] = ppl
            loc[i, a, ppl + 2:] = g.uniform(-0.15, 0.15) * np.arange(ppl)
    return torch.from_numpy(cls).cuda(), torch.from_numpy(loc).cuda()


def host_filter(lanes, mask, f):
    """the contract's counts on the host: every segment inside its own box (tests/lane_seg_filter_ref.py paints full frames)"""
    from tests import lane_seg_filter_ref as R
    H, W = mask.shape
    r = f.line_width // 2 + 1
    cls = mask == f.lane_class
    out = []
    for ln in lanes[:f.top_k]:
        xs = np.clip(np.rint(np.array([p.x for p in ln.lane], np.float64)), -R.LIM, R.LIM).astype(np.int64)
        ys = np.array([p.y for p in ln.lane], np.int64)
        m = np.zeros((H, W), bool)
        for k in range(len(xs) - 1):
            x0, x1 = max(min(xs[k], xs[k + 1]) - r, 0), min(max(xs[k], xs[k + 1]) + r, W - 1)
            y0, y1 = max(min(ys[k], ys[k + 1]) - r, 0), min(max(ys[k], ys[k + 1]) + r, H - 1)
            if x0 > x1 or y0 > y1:
                continue
            gy, gx = np.mgrid[y0:y1 + 1, x0:x1 + 1].astype(np.int64)
            m[y0:y1 + 1, x0:x1 + 1] |= R.segment_mask(int(xs[k]), int(ys[k]), int(xs[k + 1]), int(ys[k + 1]), f.line_width, gx, gy)
        area, inter = int(m.sum()), int((m & cls).sum())
        out.append({"area": area, "overlap": inter, "kept": R.decide(inter, area, f.min_ratio)})
    return out


def median_ms(fn, repeats, events):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(repeats):
        if events:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        else:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(ts))


def bench_demo(result, repeats, with_filter):
    import yaml
    from multitask_hydranet_amd import demo as DM
    cfgs = yaml.safe_load(open(os.path.join(ROOT, "cfgs", "hydranet_big.yml")))
    torch.manual_seed(0)
    demo = DM.Demo(cfgs)
    demo.det_conf = 0.95                                                 # random weights: see demo.main
    h, w, b = 720, 1280, 8
    frames = DM.synthetic_frames(b, h, w, seed=2)
    data = torch.from_numpy(frames.reshape(-1)).cuda()

    def group(**kw):
        packed = {"data": data.clone(), "offsets": h * w * 3 * np.arange(b, dtype=np.int64), "shapes": np.array([[h, w]] * b, np.int64)}
        return demo.process_device_batch(packed, **kw)

    result["demo_group_off_wall_ms"] = median_ms(lambda: group(), repeats, events=False)
    print("demo     : %8.2f ms per group of %d frames of %dx%d, the switch off (wall)" % (result["demo_group_off_wall_ms"], b, w, h))
    if with_filter:
        demo.lane_conf = 0.4                                             # random weights score every anchor near 0.5: lanes to filter
        result["demo_group_lowconf_off_wall_ms"] = median_ms(lambda: group(), repeats, events=False)
        result["demo_group_lowconf_on_wall_ms"] = median_ms(lambda: group(lane_seg_filter=True), repeats, events=False)
        r = group(lane_seg_filter=True)
        result["demo_selected_lanes"] = [len(s) for s in r["lane_filter"]]
        print("demo     : %8.2f ms off / %8.2f ms on with lane_conf 0.4 (wall); selected lanes per frame %s"
              % (result["demo_group_lowconf_off_wall_ms"], result["demo_group_lowconf_on_wall_ms"], result["demo_selected_lanes"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=16)
    ap.add_argument("--lanes", type=int, default=14)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--demo", action="store_true", help="also time Demo.process_device_batch with the switch off and on")
    ap.add_argument("--demo-only", action="store_true", help="only Demo.process_device_batch with the switch off (runs at the parent too)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_lane_seg_filter.py measures the MI355X"
    import __graft_entry__ as g
    g.build()
    result = dict(images=args.images, lanes=args.lanes, size=args.size)
    if args.demo_only:
        bench_demo(result, max(3, args.repeats // 2), with_filter=False)
        print(json.dumps(result))
        return
    from multitask_hydranet_amd import lane_codec as LC
    from multitask_hydranet_amd._lib import lib

    n, S = args.images, args.size
    codec = LC.LaneCodec(S, S, 32, S // 8)
    f = LC.LaneSegFilter(top_k=args.lanes)
    cls, loc = head_outputs(n, args.lanes, codec)
    mask_h = np.stack([label_like(S, S, 100 + k) for k in range(n)])
    mask = torch.from_numpy(mask_h).cuda()
    conf, nms = 0.5, 1
    plain = LC.decode_batch(cls, loc, codec, conf, nms, False)
    lanes, stats = LC.decode_batch(cls, loc, codec, conf, nms, False, seg_mask=mask, seg_filter=f, return_stats=True)
    result["selected_per_image"] = sorted({len(s) for s in stats})
    result["kept_lanes"] = int(sum(len(l) for l in lanes))
    assert result["selected_per_image"] == [args.lanes], result["selected_per_image"]

    # (a) the filter's launches alone, on the decode's device arrays
    hw, ppl = codec.feature_size, codec.points_per_line
    X = torch.empty((n, hw, ppl), device="cuda")
    prob = torch.empty((n, hw), device="cuda")
    ints = torch.empty((5, n, hw), device="cuda", dtype=torch.int32)
    counts = torch.empty((n,), device="cuda", dtype=torch.int32)
    lib().call("hn_lane_decode_nms", cls.data_ptr(), loc.data_ptr(), n, S, S, 32, ppl, conf, float(nms), 0, 100.0, X.data_ptr(), prob.data_ptr(),
               ints[0].data_ptr(), ints[1].data_ptr(), ints[2].data_ptr(), ints[3].data_ptr(), counts.data_ptr())
    result["filter_launches_event_ms"] = median_ms(lambda: LC._launch_seg_filter(X, ints, counts, n, S, S, 32, ppl, 8, mask, f), args.repeats, True)
    print("filter   : %8.3f ms launch sequence (HIP events), %d images of %dx%d, %d lanes each" % (result["filter_launches_event_ms"], n, S, S, args.lanes))

    # (b) decode_batch end to end
    result["decode_batch_wall_ms"] = median_ms(lambda: LC.decode_batch(cls, loc, codec, conf, nms, False), args.repeats, False)
    result["decode_batch_filter_wall_ms"] = median_ms(
        lambda: LC.decode_batch(cls, loc, codec, conf, nms, False, seg_mask=mask, seg_filter=f, return_stats=True), args.repeats, False)
    print("decode   : %8.3f ms decode_batch, %8.3f ms with the filter (wall, with the readback and the Lane objects)"
          % (result["decode_batch_wall_ms"], result["decode_batch_filter_wall_ms"]))

    # (c) the host's way: the maps come back, numpy paints
    def host():
        t0 = time.perf_counter()
        arr = mask.cpu().numpy()
        t1 = time.perf_counter()
        out = [host_filter(plain[i], arr[i], f) for i in range(n)]
        return 1e3 * (t1 - t0), 1e3 * (time.perf_counter() - t1), out
    host()
    runs = [host() for _ in range(3)]
    result["host_map_copy_wall_ms"] = float(np.median([r[0] for r in runs]))
    result["host_numpy_wall_ms"] = float(np.median([r[1] for r in runs]))
    same = all([{k: s[k] for k in ("area", "overlap", "kept")} for s in stats[i]] == runs[0][2][i] for i in range(n))
    result["host_counts_equal_device"] = bool(same)
    print("host     : %8.2f ms to copy the maps back, %8.2f ms numpy on one core; counts equal the device's: %s"
          % (result["host_map_copy_wall_ms"], result["host_numpy_wall_ms"], same))
    assert same
    if args.demo:
        bench_demo(result, max(3, args.repeats // 2), with_filter=True)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
