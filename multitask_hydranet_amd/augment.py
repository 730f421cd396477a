"""Multitask training batches assembled and augmented on the device: the per-pixel half of the reference's MultitaskData.prepare_img +
Collater (model/dataset/dataloader.py:44-162,258-380,544-633) as three HIP launches (hn_augment.hip), for a whole ragged batch of source
frames.  The host samples a small plan per image, composes its geometry into one affine map, transforms the few label coordinates and packs
the frames; everything per pixel runs on the GPU.  The result is the Collater contract that HydraTrainer.to_gpu consumes.

Semantics (imgaug and cv2 are not dependencies of this project, so this module defines them; tests/augment_ref.py restates them in float64
numpy):

Plan (sample_plan; numpy Generator seeded from (base_seed, epoch, sample index) only, so independent of DataLoader workers).  The structure
of _lane_argue with do_split=False (a tuple is a uniform range, a list a choice):
  * Sometimes(0.6) photometric op, one of 7 (1/7 each): Gaussian blur sigma ~ U(0.5, 1.5); linear contrast alpha = 1.5; multiply by
    U(0.8, 1.2), drawn per channel with probability 0.2; additive Gaussian noise, scale ~ U(0, 25.5), drawn per channel with probability 0.5;
    HSV channel 0 x U(0.7, 1.3); channel 1 x U(0.1, 2); channel 2 x U(0.5, 1.5).
  * Sometimes(0.6) geometry: 4 of [flip left-right, translate x by an integer in [-16, 16] px, shear x U(-15, 15) deg, rotate U(-15, 15)
    deg, (flip up-down when dataloader.do_flip), crop-and-keep-size (top {0, 0.2}, right {0, 0.15}, bottom 0, left {0, 0.15})], applied in
    list order.  with_aug False and mode "val" give the identity plan.
With dataloader.do_split and a split ratio r (cal_split; a ratio of None takes the structure above, draw for draw; no ratio given at all
raises NotImplementedError), the structure of _lane_argue with do_split=True:
  * the photometric op as above;
  * Sometimes(0.6) split: one of two keep-size crops (1/2 each), as (T, R, B, L) fractions: split_one (top {0, 0.2}, right 1 - r,
    bottom 0, left {0, 0.15}); split_two (top {0, 0.2}, right {0, 0.15}, bottom 0, left r);
  * Sometimes(0.6) position: 4 of [flip left-right, translate x, shear x, rotate, (flip up-down when do_flip)], no crop, in list order;
  * one uniform draw (made whether or not the blocks apply) of whether the split comes before or after the position block.

Coordinates are continuous, pixel (i, j) covers [j, j+1) x [i, i+1).  The chosen ops compose into one forward affine F (source ->
augmented frame, same size as the source).  Single ops, about the centre (cx, cy) = (W/2, H/2):
  flip lr x -> W - x;  flip ud y -> H - y;  translate x -> x + t;  shear x -> x + tan(a) (y - cy);
  rotate (x, y) -> c + R(a) (p - c) with R = [[cos a, -sin a], [sin a, cos a]] (positive a turns clockwise on screen, y pointing down);
  crop (T, R, B, L px = rint(fraction * size)) x -> (x - L) W / (W - L - R), y -> (y - T) H / (H - T - B).
  crop clamp: a negative fraction is 0; if L + R >= W, L and R give back g = L + R - W + 1 px, ceil(g / 2) from L and floor(g / 2) from R,
    a side that has too little giving all it has and the other the rest (T, B alike, T first), so 1 px remains (imgaug keeps 1 px too).

Image:
  1. the photometric op at source resolution on the BGR buffer as loaded; the HSV ops read it as RGB (as the reference hands cv2's BGR array
     to imgaug), OpenCV's 8-bit RGB->HSV (H in [0, 180), hsv_shift 12) and float HSV->RGB; the hue wraps mod 180 after the multiply.  Every
     op ends in rint (half to even) + clamp to uint8.  Blur: separable, radius = ((rint(6 sigma + 1)) | 1) // 2 (OpenCV's 8-bit kernel
     size from sigma), weights exp(-k^2 / 2 sigma^2) normalised in float64 then fp32, horizontal pass then vertical pass in fp32 (tap order
     -r..r), reflect-101 border.  Contrast 127.5 + alpha (v - 127.5), multiply v f, in float64.  Noise: Philox4x32-10, key = the plan's
     64-bit noise seed, counter = (pixel index y W + x as two 32-bit words, 0, 0); u1 = (w0 + 1) / 2^32, u2 = w1 / 2^32, u3 = (w2 + 1) / 2^32,
     u4 = w3 / 2^32; channel c of a per-channel draw takes z = [r1 cos t2, r1 sin t2, r3 cos t4][c] (r = sqrt(-2 ln u), t = 2 pi u), one
     shared draw takes z0; v + scale z in float64.
  2. warp: augmented-frame pixel centre (x + 0.5, y + 0.5) -> F^-1 -> bilinear in pixel-centre space (taps outside the frame are 0),
     float64, rint + clamp: the intermediate frame at source size (never stored).
  3. INTER_AREA to the network size, OpenCV's algorithm: scale = 1 / (Wd / Ws); integer scales on both axes take resizeAreaFast (block
     sum x (1/area) in fp32), others resizeArea (computeResizeAreaTab; per source row the alpha-weighted fp32 sum in tap order, then the
     beta-weighted sum over rows); rint + clamp.  A source smaller than the network input on either axis is a ValueError.
  4. BGR->RGB, (v / 255 - mean) / std in float64, fp32 NCHW (as hn_preprocess_bgr).
Seg map (uint8, source size): output (x, y) picks intermediate pixel (floor(x / (Wd / Ws)), floor(y / (Hd / Hs))) (INTER_NEAREST), its
  centre through F^-1, floor to a source pixel, 0 outside.
Boxes (float64): the axis-aligned hull of F(4 corners); boxes with no overlap with (0, W) x (0, H) are dropped, the rest clipped to
  [0, W] x [0, H]; scaled by (Wd / Ws, Hd / Hs); padded with -1 rows to the batch maximum (at least one row); fp32 [N, M, 5].
Lanes: F on every point, then float(int(.)) (truncation toward zero, no clipping), as annot_lane JSON with src_image_shape = source size.
An image whose plan is not augmented (val, with_aug False) keeps its boxes and lanes exactly as parsed.

Deviations from the reference (imgaug), one line each:
  * imgaug runs the photometric and geometric blocks in random order; here the photometric op always comes first, at source resolution.
  * with a split, imgaug's random_order over three blocks becomes one draw of the order of the split and position blocks.
  * imgaug resamples once per geometric op (the keep-size crop by its documented default cubic); here the ops compose into one bilinear warp.
  * the integer-factor INTER_AREA path rounds half to even everywhere (OpenCV's SIMD 2x2 specialisation rounds halves up).
  * the label map is resized with INTER_NEAREST; the reference's Collater passes the flag in cv2.resize's dst slot and so resizes bilinearly.
  * box clipping and dropping use the plain frame [0, W] x [0, H]; noise is Philox + Box-Muller; blur is fp32 separable, not fixed point.
"""
from __future__ import annotations

import json
import math
import warnings
from typing import List, Optional, Sequence

import numpy as np
import torch

from ._lib import lib

PHOTO_OPS = ("none", "blur", "contrast", "multiply", "noise", "hue", "sat", "val")
HSV_RANGES = {"hue": (0.7, 1.3), "sat": (0.1, 2.0), "val": (0.5, 1.5)}
MAX_BLUR_RADIUS = 7

# hn_augment.hip struct AugDesc
DESC_DTYPE = np.dtype({
    "names": ["finv", "p", "src_off", "ws_off", "seg_off", "Hs", "Ws", "op", "per_channel", "seed_lo", "seed_hi", "radius", "w"],
    "formats": [("<f8", 6), ("<f8", 4), "<i8", "<i8", "<i8", "<i4", "<i4", "<i4", "<i4", "<u4", "<u4", "<i4", ("<f4", 8)],
    "offsets": [0, 48, 80, 88, 96, 104, 108, 112, 116, 120, 124, 128, 136],
    "itemsize": 176})


# ---- plans ------------------------------------------------------------------------------------------------------------------------
def identity_plan() -> dict:
    return {"augmented": False, "photo": None, "geom": [], "seed": 0}


def cal_split(lanes: dict, width: int, height: int):
    """MultitaskData.cal_split (dataloader.py:428-480) on a parsed lane dict ({"Lines": [[{"x", "y"}, ...]]}) of a width x height source
    -> (split possible, split ratio or None), every quirk of the reference kept"""
    k1, all_lines = [], []
    for line in lanes["Lines"]:
        # a point is (int(float(x)), height - int(float(y))): truncation toward zero, y flipped
        pts = [(int(float(pt["x"])), height - int(float(pt["y"]))) for pt in line]
        with warnings.catch_warnings():
            # any warning (RankWarning of a vertical, one-point or degenerate lane) or exception of any lane: no split.  The reference's
            # `except np.RankWarning` fails itself under numpy 2; this is its numpy-1 meaning
            warnings.filterwarnings("error")
            try:
                coeff = np.polyfit([q[0] for q in pts], [q[1] for q in pts], 1)
            except Exception:
                return False, None
        k1.append(coeff[0])
        all_lines.append(pts)
    k1 = np.array(k1)
    sorted_k1 = np.sort(k1)
    index = np.argsort(k1)
    # the reference's misplaced parenthesis: np.all(sorted_k1) <= 0 is true exactly when some slope is exactly 0 (no lanes: the first term)
    if np.all(sorted_k1 >= 0) or np.all(sorted_k1) <= 0:
        return False, None
    left = np.array(all_lines[index[np.where(sorted_k1 <= 0)[0][0]]])        # the most negative slope
    right = np.array(all_lines[index[-1]])                                     # the largest slope
    # each lane's points sorted by the flipped y (np.argsort, as the reference), the x of the first
    left_x = left[np.argsort(left[:, 1], axis=0)][0, 0]
    right_x = right[np.argsort(right[:, 1], axis=0)][0, 0]
    return True, float((left_x + right_x) / 2.0 / width)


_POSITION_OPS = ["fliplr", "translate_x", "shear_x", "rotate"]


def _position_ops(rng, names: List[str]) -> list:
    """4 of `names` (SomeOf(4)), in list order, with their parameters"""
    ops = []
    for i in np.sort(rng.choice(len(names), 4, replace=False)):
        name = names[i]
        if name == "translate_x":
            ops.append((name, int(rng.integers(-16, 17))))
        elif name in ("shear_x", "rotate"):
            ops.append((name, float(rng.uniform(-15.0, 15.0))))
        elif name == "crop":
            ops.append((name, (float(rng.choice([0.0, 0.2])), float(rng.choice([0.0, 0.15])), 0.0, float(rng.choice([0.0, 0.15])))))
        else:
            ops.append((name, None))
    return ops


NO_RATIO = object()           # sample_plan's split_ratio when the caller gave none (None is an answer: the image's lanes give no split)


def sample_plan(base_seed: int, epoch: int, index: int, with_aug: bool = True, do_flip: bool = False, do_split: bool = False,
                split_ratio=NO_RATIO) -> dict:
    """one image's plan, a function of (base_seed, epoch, index) (and the image's split ratio) alone.  do_split needs split_ratio, the
    image's cal_split ratio or None when it has none.  A split plan (do_split with a ratio) also carries plan["split"] = {"ratio", "crop":
    "one" / "two" / None (block not applied), "split_first"}; every other plan is drawn exactly as without do_split."""
    if do_split and split_ratio is NO_RATIO:
        raise NotImplementedError("sample_plan(do_split=True) without split_ratio: a split plan needs the image's split ratio "
                                  "(augment.cal_split of its lanes; None when they give none)")
    if split_ratio is NO_RATIO:
        split_ratio = None
    if not with_aug:
        return identity_plan()
    rng = np.random.default_rng([int(base_seed), int(epoch), int(index)])
    plan = {"augmented": True, "photo": None, "geom": [], "seed": int(rng.integers(0, 2 ** 63, dtype=np.int64))}
    if rng.random() < 0.6:
        k = int(rng.integers(7))
        name = PHOTO_OPS[1 + k]
        if name == "blur":
            plan["photo"] = {"op": name, "sigma": float(rng.uniform(0.5, 1.5))}
        elif name == "contrast":
            plan["photo"] = {"op": name, "alpha": 1.5}
        elif name == "multiply":
            pc = bool(rng.random() < 0.2)
            f = rng.uniform(0.8, 1.2, size=3 if pc else 1)
            plan["photo"] = {"op": name, "per_channel": pc, "factor": [float(v) for v in (f if pc else np.repeat(f, 3))]}
        elif name == "noise":
            pc = bool(rng.random() < 0.5)
            plan["photo"] = {"op": name, "per_channel": pc, "scale": float(rng.uniform(0.0, 25.5))}
        else:
            lo, hi = HSV_RANGES[name]
            plan["photo"] = {"op": name, "factor": float(rng.uniform(lo, hi))}
    names = _POSITION_OPS + (["flipud"] if do_flip else [])
    if not (do_split and split_ratio is not None):
        if rng.random() < 0.6:
            plan["geom"] = _position_ops(rng, names + ["crop"])
        return plan
    r = float(split_ratio)
    split = {"ratio": r, "crop": None, "split_first": False}
    crop = []
    if rng.random() < 0.6:
        split["crop"] = ("one", "two")[int(rng.integers(2))]
        top, other = float(rng.choice([0.0, 0.2])), float(rng.choice([0.0, 0.15]))
        crop = [("crop", (top, 1.0 - r, 0.0, other) if split["crop"] == "one" else (top, other, 0.0, r))]
    position = _position_ops(rng, names) if rng.random() < 0.6 else []
    split["split_first"] = bool(rng.random() < 0.5)
    plan["geom"] = crop + position if split["split_first"] else position + crop
    plan["split"] = split
    return plan


def _keep_one(a: int, b: int, size: int):
    """crop amounts a (top / left) and b (bottom / right) of one axis, reduced so that at least 1 px of `size` remains"""
    g = a + b - size + 1
    if g <= 0:
        return a, b
    ga, gb = (g + 1) // 2, g // 2
    if ga > a:
        ga, gb = a, g - a
    elif gb > b:
        ga, gb = g - b, b
    return a - ga, b - gb


def crop_pixels(param, W: int, H: int):
    """(T, R, B, L) fractions -> pixels: rint(max(fraction, 0) * size), then the 1 px clamp of the module docstring"""
    top, right, bottom, left = (max(float(v), 0.0) for v in param)
    T, R, B, L = (int(np.rint(top * H)), int(np.rint(right * W)), int(np.rint(bottom * H)), int(np.rint(left * W)))
    T, B = _keep_one(T, B, H)
    L, R = _keep_one(L, R, W)
    return T, R, B, L


def op_matrix(name: str, param, W: int, H: int) -> np.ndarray:
    """3x3 forward matrix of one geometric op on a W x H frame"""
    cx, cy = W / 2.0, H / 2.0
    M = np.eye(3)
    if name == "fliplr":
        M[0, 0], M[0, 2] = -1.0, float(W)
    elif name == "flipud":
        M[1, 1], M[1, 2] = -1.0, float(H)
    elif name == "translate_x":
        M[0, 2] = float(param)
    elif name == "shear_x":
        t = math.tan(math.radians(param))
        M[0, 1], M[0, 2] = t, -t * cy
    elif name == "rotate":
        a = math.radians(param)
        c, s = math.cos(a), math.sin(a)
        M[:2, :2] = [[c, -s], [s, c]]
        M[0, 2] = cx - c * cx + s * cy
        M[1, 2] = cy - s * cx - c * cy
    elif name == "crop":
        T, R, B, L = crop_pixels(param, W, H)
        sx, sy = W / float(W - L - R), H / float(H - T - B)
        M[0, 0], M[0, 2] = sx, -L * sx
        M[1, 1], M[1, 2] = sy, -T * sy
    else:
        raise ValueError("unknown geometric op %r" % (name,))
    return M


def forward_matrix(plan: dict, W: int, H: int) -> np.ndarray:
    """F (3x3, source -> augmented frame): the plan's geometric ops composed in list order"""
    F = np.eye(3)
    for name, param in plan["geom"]:
        F = op_matrix(name, param, W, H) @ F
    return F


def blur_weights(sigma: float):
    r = (int(np.rint(sigma * 6 + 1)) | 1) // 2
    k = np.arange(-r, r + 1, dtype=np.float64)
    w = np.exp(-(k * k) / (2.0 * sigma * sigma))
    w = w / w.sum()
    return r, w[r:].astype(np.float32)


# ---- labels -----------------------------------------------------------------------------------------------------------------------
def transform_boxes(det: np.ndarray, F: np.ndarray, W: int, H: int) -> np.ndarray:
    """[k, 5] x1, y1, x2, y2, class (float64) -> the augmented frame's boxes (hull of the 4 mapped corners, fully outside dropped, clipped)"""
    det = np.asarray(det, dtype=np.float64).reshape(-1, 5)
    if det.shape[0] == 0:
        return det.copy()
    xs = det[:, [0, 2, 2, 0]]
    ys = det[:, [1, 1, 3, 3]]
    tx = F[0, 0] * xs + F[0, 1] * ys + F[0, 2]
    ty = F[1, 0] * xs + F[1, 1] * ys + F[1, 2]
    out = np.stack([tx.min(1), ty.min(1), tx.max(1), ty.max(1), det[:, 4]], axis=1)
    keep = (out[:, 0] < W) & (out[:, 2] > 0) & (out[:, 1] < H) & (out[:, 3] > 0)
    out = out[keep]
    out[:, [0, 2]] = np.clip(out[:, [0, 2]], 0.0, float(W))
    out[:, [1, 3]] = np.clip(out[:, [1, 3]], 0.0, float(H))
    return out


def transform_lanes(lane: dict, F: np.ndarray) -> dict:
    """F on every lane point, then float(int(.)) (dataloader.py:138-143); Labels None as the reference's augmented lanes"""
    lines = []
    for line in lane["Lines"]:
        if not line:
            lines.append([])
            continue
        p = np.array([[float(pt["x"]), float(pt["y"])] for pt in line], dtype=np.float64)
        x = F[0, 0] * p[:, 0] + F[0, 1] * p[:, 1] + F[0, 2]
        y = F[1, 0] * p[:, 0] + F[1, 1] * p[:, 1] + F[1, 2]
        lines.append([{"x": float(int(a)), "y": float(int(b))} for a, b in zip(x.tolist(), y.tolist())])
    return {"Lines": lines, "Labels": None}


def pad_boxes(dets: Sequence[np.ndarray], scales) -> np.ndarray:
    """Collater: scale by (Wd / Ws, Hd / Hs) and pad with -1 rows to the batch maximum (at least one row) -> fp32 [N, M, 5]"""
    m = max([1] + [d.shape[0] for d in dets])
    out = np.full((len(dets), m, 5), -1.0, dtype=np.float32)
    for i, (d, (sx, sy)) in enumerate(zip(dets, scales)):
        if d.shape[0]:
            d = d.copy()
            d[:, :4] *= np.array([sx, sy, sx, sy])
            out[i, :d.shape[0]] = d
    return out


# ---- packing ----------------------------------------------------------------------------------------------------------------------
def pack(arrays: Sequence[np.ndarray], pin: bool = False) -> dict:
    """a ragged list of uint8 arrays (H x W x 3 frames or H x W label maps) -> one flat uint8 tensor + byte offsets + (H, W) per image"""
    sizes = [int(a.nbytes) for a in arrays]
    offs = np.zeros(len(arrays) + 1, dtype=np.int64)
    offs[1:] = np.cumsum(sizes)
    data = torch.empty((max(1, int(offs[-1])),), dtype=torch.uint8, pin_memory=pin)
    buf = data.numpy()
    for a, o, s in zip(arrays, offs[:-1], sizes):
        assert a.dtype == np.uint8, a.dtype
        buf[o:o + s] = np.ascontiguousarray(a).reshape(-1)
    shapes = np.array([a.shape[:2] for a in arrays], dtype=np.int64).reshape(-1, 2)
    return {"data": data, "offsets": offs[:-1].copy(), "shapes": shapes}


def _as_packed(x):
    if x is None or isinstance(x, dict):
        return x
    return pack([np.asarray(a) for a in x])


def describe(plan: dict, W: int, H: int) -> dict:
    """the device descriptor's content of one image: F, F^-1 and the photometric op's code + parameters"""
    F = forward_matrix(plan, W, H)
    Finv = np.linalg.inv(F)
    ph = plan.get("photo")
    d = {"F": F, "finv": Finv[:2].reshape(-1), "op": 0, "p": np.zeros(4), "per_channel": 0, "seed": int(plan.get("seed", 0)), "radius": 0,
         "w": np.zeros(8, np.float32)}
    if ph is not None:
        d["op"] = PHOTO_OPS.index(ph["op"])
        if ph["op"] == "blur":
            r, w = blur_weights(ph["sigma"])
            assert r <= MAX_BLUR_RADIUS
            d["radius"], d["w"][:r + 1] = r, w
        elif ph["op"] == "contrast":
            d["p"][0] = ph["alpha"]
        elif ph["op"] == "multiply":
            d["p"][:3] = ph["factor"]
            d["per_channel"] = int(ph["per_channel"])
        elif ph["op"] == "noise":
            d["p"][0] = ph["scale"]
            d["per_channel"] = int(ph["per_channel"])
        else:
            d["p"][0] = ph["factor"]
    return d


def augment_batch(frames, lanes: Optional[List[dict]], boxes: Optional[List[np.ndarray]], segs, plans: List[dict], out_hw, device=None) -> dict:
    """frames: list of uint8 BGR H x W x 3 arrays or pack()'s dict (pin its buffer for an asynchronous upload); lanes: parsed lane dicts
    ({"Lines": [[{"x", "y"}, ...]], "Labels"}) or None; boxes: [k, 5] xyxy + class arrays or None; segs: uint8 H x W label maps (list or
    packed) or None; plans: one per image.  -> the Collater contract on `device`: image fp32 [N, 3, Hd, Wd], gt_seg uint8 [N, Hd, Wd],
    gt_det fp32 [N, M, 5], annot_lane (JSON per image), src_image_shape, net_input_image_shape."""
    fr = _as_packed(frames)
    sg = _as_packed(segs)
    n = len(plans)
    shapes = fr["shapes"]
    assert shapes.shape[0] == n, (shapes.shape, n)
    hd, wd = int(out_hw[0]), int(out_hw[1])
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    if sg is not None and not np.array_equal(sg["shapes"], shapes):
        raise ValueError("every label map must have its frame's size")
    desc = np.zeros(n, dtype=DESC_DTYPE)
    ws_total = 0
    fr_bytes = int(fr["data"].numel())
    dets, lane_out, scales = [], [], []
    for i, plan in enumerate(plans):
        H, W = int(shapes[i, 0]), int(shapes[i, 1])
        if H < hd or W < wd:
            raise ValueError("source frame %dx%d is smaller than the network input %dx%d (INTER_AREA does not upscale)" % (W, H, wd, hd))
        assert int(fr["offsets"][i]) + H * W * 3 <= fr_bytes
        d = describe(plan, W, H)
        e = desc[i]
        e["finv"], e["p"], e["op"], e["per_channel"], e["radius"], e["w"] = d["finv"], d["p"], d["op"], d["per_channel"], d["radius"], d["w"]
        e["seed_lo"], e["seed_hi"] = d["seed"] & 0xFFFFFFFF, (d["seed"] >> 32) & 0xFFFFFFFF
        e["Hs"], e["Ws"], e["src_off"] = H, W, int(fr["offsets"][i])
        e["seg_off"] = int(sg["offsets"][i]) if sg is not None else -1
        if d["op"]:
            e["ws_off"] = ws_total
            ws_total += H * W * 3
        else:
            e["ws_off"] = -1
        scales.append((wd / float(W), hd / float(H)))
        if boxes is not None:
            b = np.asarray(boxes[i], dtype=np.float64).reshape(-1, 5)
            dets.append(transform_boxes(b, d["F"], W, H) if plan["augmented"] else b.copy())
        if lanes is not None:
            lane_out.append(transform_lanes(lanes[i], d["F"]) if plan["augmented"] else lanes[i])
    src = fr["data"].to(dev, non_blocking=fr["data"].is_pinned())
    desc_d = torch.from_numpy(desc.view(np.uint8).copy()).to(dev)
    img = torch.empty((n, 3, hd, wd), device=dev, dtype=torch.float32)
    L = lib()
    with torch.cuda.device(dev):
        ws = torch.empty((max(1, ws_total),), device=dev, dtype=torch.uint8)
        if ws_total:
            L.call("hn_augment_photometric", src.data_ptr(), desc_d.data_ptr(), n, int(shapes[:, 0].max()), int(shapes[:, 1].max()), ws.data_ptr())
        L.call("hn_augment_image", src.data_ptr(), ws.data_ptr(), desc_d.data_ptr(), n, hd, wd, img.data_ptr())
        out = {"image": img,
               "src_image_shape": [{"width": int(shapes[i, 1]), "height": int(shapes[i, 0]), "channel": 3} for i in range(n)],
               "net_input_image_shape": [json.dumps(dict(width=wd, height=hd, channel=3))] * n}
        if sg is not None:
            assert all(int(sg["offsets"][i]) + int(shapes[i, 0] * shapes[i, 1]) <= int(sg["data"].numel()) for i in range(n))
            seg_src = sg["data"].to(dev, non_blocking=sg["data"].is_pinned())
            gseg = torch.empty((n, hd, wd), device=dev, dtype=torch.uint8)
            L.call("hn_augment_seg", seg_src.data_ptr(), desc_d.data_ptr(), n, hd, wd, gseg.data_ptr())
            out["gt_seg"] = gseg
    if boxes is not None:
        out["gt_det"] = torch.from_numpy(pad_boxes(dets, scales)).to(dev)
    if lanes is not None:
        out["annot_lane"] = [json.dumps(l) for l in lane_out]
    return out
