"""Lane ground-truth encoding, lane decode + lane NMS on the device (reference: head_lane/lanedetect.py:103-125 LaneHeader.decode / scale_to_org,
head_lane/lane_codec.py:25-51,116-219 LaneCodec.decode_lane, head_lane/lane_codec_utils.py:6-64,185-282,487-543).

`decode(predict_cls, predict_loc, pointlane, conf_thres, nms_line_thres, use_mean)` keeps the reference's signature and return type (a list
of Lane objects in descending-probability order); the per-anchor point walk, the stable probability sort and the greedy distance NMS run
in ONE kernel launch for the whole batch (hn_lane_decode_nms, one workgroup per image).  `pointlane` may be the reference's own LaneCodec
object or this module's LaneCodec (only the geometry fields are read).  scale_to_org / order_lane_x_axis / convert_lane_to_dict are the
host-side bookkeeping on the handful of surviving lanes, restated.

`LaneCodec.encode_lane` / `encode_lanes` (reference: head_lane/lane_codec.py:53-114,221-366, lane_spline_interp.py, and the dataset's
division, dataset/dataloader.py:343-352): the host parses and packs the annotations (`pack_lanes`), hn_lane_encode does the rest for the
whole batch.

`LaneSegFilter` with `decode(..., seg_mask=, seg_filter=)` / `decode_batch`: the deploy path's cross-head step (deploy/src/model/
hydranet_model.cpp:546-607) -- the NMS survivors capped at top_k and filtered by their overlap with the seg head's marking class -- on the
device between the decode and its one readback (hn_lane_seg_filter).  Off unless a filter is passed.
"""
from __future__ import annotations

import dataclasses
import json
from typing import List

import numpy as np
import torch

from ._lib import lib


class Point:
    def __init__(self, x=0, y=0):
        self.x, self.y = x, y

    def __repr__(self):
        return "{}, {}".format(self.x, self.y)


class Lane:
    def __init__(self, prob=0, start_pos=0, end_pos=0, anchor_x=0, anchor_y=0, type=0, lane=None):
        self.prob, self.start_pos, self.end_pos = prob, start_pos, end_pos
        self.lane = lane if lane is not None else np.array([])
        self.idx, self.ax, self.ay, self.type = 0, anchor_x, anchor_y, type

    def __lt__(self, other):
        return self.prob > other.prob


class LaneCodec:
    """the reference's LaneCodec (lane_codec.py:25-51): its geometry, encode_lane / encode_lanes (ground-truth generation on the device,
    hn_lane_encode) and decode_lane"""

    def __init__(self, input_width, input_height, anchor_stride, points_per_line, do_interpolate=False, anchor_lane_num=1,
                 scale_invariance=True):
        self.input_width, self.input_height, self.stride = input_width, input_height, anchor_stride
        self.feature_width, self.feature_height = int(input_width / anchor_stride), int(input_height / anchor_stride)
        self.points_per_line = points_per_line
        self.pt_nums_single_lane = 2 * points_per_line + 2
        self.points_per_anchor = points_per_line / self.feature_height
        self.interval = float(input_height) / points_per_line
        self.feature_size = self.feature_width * self.feature_height
        self.step_w = self.step_h = anchor_stride
        self.anchor_lane_num, self.interpolation, self.scale_invariance = anchor_lane_num, do_interpolate, scale_invariance

    def encode_lane(self, lane_object, org_width, org_height):
        """LaneCodec.encode_lane (lane_codec.py:53-114) for ONE image: numpy fp32 (gt_type [F, 2], gt_loc [F, 2P+2]) BEFORE the dataset's
        scale-invariance division; (None, None) when anchor_lane_num != 1, as the reference"""
        if self.anchor_lane_num != 1:
            return None, None
        cls, loc = self.encode_lanes([lane_object], [(org_width, org_height)], divide=False)
        return cls[0].cpu().numpy(), loc[0].cpu().numpy()

    def encode_lanes(self, lane_objects, org_sizes, device=None, div_interval=None, divide=True):
        """the batched device encoder: torch fp32 (gt_cls [N, F, 2], gt_loc [N, F, 2P+2]) on `device` in the dataset's final form
        (dataloader.py:343-352: columns [0, P) and [P+2, 2P+2) divided by `div_interval` (default: the codec's interval) when
        scale_invariance).  lane_objects: JSON strings or {"Lines": ...} dicts; org_sizes: (width, height) pairs or {"width", "height"}
        dicts / JSON strings.  The host only parses and packs; everything after the parse is one call (two launches), no synchronisation."""
        if self.anchor_lane_num != 1:
            raise ValueError("lane ground-truth encoding exists for anchor_lane_num == 1 only (the reference encodes no other)")
        dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        W, H, stride, P = int(self.input_width), int(self.input_height), int(self.stride), int(self.points_per_line)
        pts, ints, n_lanes = pack_lanes(lane_objects, org_sizes, W, H, self.interval, self.interpolation, P)
        n = len(lane_objects)
        pts_d = torch.from_numpy(pts).pin_memory().to(dev, non_blocking=True)
        ints_d = torch.from_numpy(ints).pin_memory().to(dev, non_blocking=True)
        F = self.feature_size
        cls = torch.empty((n, F, 2), device=dev, dtype=torch.float32)
        loc = torch.empty((n, F, 2 * P + 2), device=dev, dtype=torch.float32)
        ws = torch.empty((lib().query("hn_lane_encode_ws_bytes", n_lanes, len(pts), W, H, stride, P),), device=dev, dtype=torch.uint8)
        si = bool(self.scale_invariance) and divide
        div = float(div_interval if div_interval is not None else self.interval)
        with torch.cuda.device(dev):
            lib().call("hn_lane_encode", pts_d.data_ptr() if len(pts) else 0, ints_d.data_ptr(), ints_d.data_ptr() + 4 * (n_lanes + 1), n,
                       n_lanes, len(pts), W, H, stride, P, int(bool(self.interpolation)), int(si), div, ws.data_ptr(), cls.data_ptr(),
                       loc.data_ptr())
        return cls, loc

    def decode_lane(self, predict_type, predict_loc, exist_threshold=0.5, margin_width=100.0):
        """candidates before NMS (LaneCodec.decode_lane takes POST-softmax probabilities): runs the device kernel with the NMS disabled"""
        logits = torch.log(predict_type.clamp_min(1e-38))
        return _decode_batch(logits[None], predict_loc[None], self, exist_threshold, -1.0, False, margin_width, keep_all=True)[0]


# ---- the host half of encode_lane: get_lane_list + trans_to_lane_with_type + delete_repeat_y (lane_codec_utils.py:127-183,285-320) ----
_MAX_SAMPLES = 1 << 24
_MAX_COORD = float(1 << 24)


def _raw_lines(lane_object, sx, sy, xs, ys, counts):
    """append one annotation's points ("nan" skipped, duplicate RAW y dropped, reversed when the first two go upward once scaled) to the
    flat lists, UNSCALED (the caller scales: the same fp64 product); the point count of every lane with >= 2 points to `counts`"""
    if isinstance(lane_object, (str, bytes)):
        lane_object = json.loads(lane_object)
    for line in lane_object["Lines"]:
        xr = [p["x"] for p in line]
        yr = [p["y"] for p in line]
        if "nan" in xr or "nan" in yr or len(set(yr)) != len(yr):
            raw_y, kx, ky = set(), [], []
            for px, py in zip(xr, yr):
                if px == "nan" or py == "nan" or py in raw_y:
                    continue
                raw_y.add(py)
                kx.append(px)
                ky.append(py)
            xr, yr = kx, ky
        if len(xr) < 2:
            continue
        lx, ly = list(map(float, xr)), list(map(float, yr))
        if ly[0] * sy < ly[1] * sy:
            lx.reverse()
            ly.reverse()
        xs += lx
        ys += ly
        counts.append(len(lx))


def _scale_sort_dedupe(xs, ys, counts, scales):
    """scale, then per lane: stable sort by descending y, the first x of every float y; lanes left with < 2 points dropped.
    -> x, y, lane id (dense over the input lanes)"""
    counts = np.array(counts, np.int64)
    lid = np.repeat(np.arange(len(counts)), counts)
    sc = np.array(scales, np.float64).reshape(-1, 2)
    x = np.array(xs, np.float64) * sc[lid, 0]
    y = np.array(ys, np.float64) * sc[lid, 1]
    inner = lid[1:] == lid[:-1]
    if not np.all(y[1:][inner] < y[:-1][inner]):                      # (already strictly descending: nothing to sort or drop)
        order = np.lexsort((np.arange(len(y)), -y, lid))
        x, y, lid = x[order], y[order], lid[order]
        keep = np.ones(len(y), bool)
        keep[1:] = (y[1:] != y[:-1]) | (lid[1:] != lid[:-1])
        x, y, lid = x[keep], y[keep], lid[keep]
        ok = np.bincount(lid, minlength=len(counts))[lid] >= 2
        x, y, lid = x[ok], y[ok], lid[ok]
    return x, y, lid


def parse_lane_object(lane_object, W, H, org_w, org_h):
    """one annotation -> [(x, y)] fp64 arrays per lane, y descending: "nan" points skipped, duplicate y dropped on the RAW value,
    scaled by W / org_w, H / org_h; the first two points decide whether the list is reversed (bottom first), then a stable sort by
    descending y keeps the first x of every float y; lanes with fewer than 2 points left are dropped"""
    xs, ys, counts = [], [], []
    sx, sy = W * 1.0 / org_w, H * 1.0 / org_h
    _raw_lines(lane_object, sx, sy, xs, ys, counts)
    x, y, lid = _scale_sort_dedupe(xs, ys, counts, [(sx, sy)] * len(counts))
    return [(x[lid == l], y[lid == l]) for l in np.unique(lid)]


def _org_size(s):
    if isinstance(s, (str, bytes)):
        s = json.loads(s)
    if isinstance(s, dict):
        return float(s["width"]), float(s["height"])
    return float(s[0]), float(s[1])


def pack_lanes(lane_objects, org_sizes, W, H, interval, interpolate, P):
    """a batch of annotations -> (pts fp64 [n_points, 2], ints int32 = lane offsets [n_lanes + 1] ++ image lane offsets [N + 1], n_lanes).
    Raises ValueError on lanes the encoder cannot take: non-finite or absurd coordinates, more than 2^24 spline samples in the batch (the
    reference would spin on them), and without `interpolate` a lane starting more than P + 1 intervals below the image (its loc rows
    would not fit the 2P + 2 columns: the reference fails on them)."""
    if len(lane_objects) != len(org_sizes):
        raise ValueError("lane_objects and org_sizes differ in length: %d vs %d" % (len(lane_objects), len(org_sizes)))
    xs, ys, counts, scales, first_lane = [], [], [], [], [0]
    for obj, sz in zip(lane_objects, org_sizes):
        ow, oh = _org_size(sz)
        sx, sy = W * 1.0 / ow, H * 1.0 / oh
        _raw_lines(obj, sx, sy, xs, ys, counts)
        scales += [(sx, sy)] * (len(counts) - first_lane[-1])
        first_lane.append(len(counts))
    x, y, lid = _scale_sort_dedupe(xs, ys, counts, scales)
    if not (np.all(np.abs(x) < _MAX_COORD) and np.all(np.abs(y) < _MAX_COORD)):
        raise ValueError("lane coordinates outside +-2^24 or not finite after scaling")
    lanes, starts = np.unique(lid, return_index=True)                # surviving lanes in order, their first point
    same = lid[1:] == lid[:-1]
    dx, dy = (x[:-1] - x[1:])[same], (y[:-1] - y[1:])[same]
    if int(np.ceil(np.sqrt(dx * dx + dy * dy)).sum()) + len(lanes) > _MAX_SAMPLES:
        raise ValueError("lane annotations of more than 2^24 spline samples in one batch")
    if not interpolate and len(lanes):
        yb = y[starts]
        if np.any(np.trunc((H - 1 - yb) / interval + 1) < -(P + 1)):
            raise ValueError("a lane starts %.1f px below the %d px input: beyond what the loc rows can hold" % (yb.max() - H, H))
    lane_off = np.zeros(len(lanes) + 1, np.int64)
    lane_off[1:] = np.cumsum(np.diff(np.append(starts, len(lid))))
    img_lane = np.searchsorted(lanes, np.array(first_lane, np.int64))  # surviving lanes before every image's first lane id
    pts = np.ascontiguousarray(np.stack([x, y], 1))
    return pts, np.concatenate([lane_off, img_lane]).astype(np.int32), len(lanes)


@dataclasses.dataclass(frozen=True)
class LaneSegFilter:
    """the deploy path's filter of the lanes the NMS leaves (deploy/src/model/hydranet_model.cpp:546-607; the defaults are the constants
    of hydranet_model.h:68-75): at most top_k lanes, each painted line_width thick and kept when more than min_ratio of its painted
    pixels lie on the seg arg-max map's lane_class (marking_area in the shipped cfgs).  DESIGN.md 4n."""
    lane_class: int = 2
    line_width: int = 20
    min_ratio: float = 0.01
    top_k: int = 14

    def __post_init__(self):
        for name in ("lane_class", "line_width", "top_k"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise ValueError("LaneSegFilter.%s is an integer, not %r" % (name, v))
        if self.lane_class < 0:
            raise ValueError("LaneSegFilter.lane_class is a class id >= 0, not %d" % self.lane_class)
        if not 1 <= self.line_width <= 16384:
            raise ValueError("LaneSegFilter.line_width is 1 .. 16384 pixels, not %d" % self.line_width)
        if not 1 <= self.top_k <= 64:
            raise ValueError("LaneSegFilter.top_k is 1 .. 64 lanes, not %d" % self.top_k)
        r = self.min_ratio
        if isinstance(r, bool) or not isinstance(r, (int, float, np.floating, np.integer)) or not np.isfinite(float(r)):
            raise ValueError("LaneSegFilter.min_ratio is a finite number, not %r" % (r,))


def _check_seg_filter(seg_mask, seg_filter, return_stats, codec, n):
    """the filter's arguments, checked before anything is launched -> the integer interval of the codec's rows"""
    if seg_filter is None:
        if return_stats:
            raise ValueError("return_stats asks for the seg filter's statistics: pass a seg_filter")
        return None
    if not isinstance(seg_filter, LaneSegFilter):
        raise ValueError("seg_filter is a LaneSegFilter (or None), not %r" % (seg_filter,))
    if seg_mask is None or not torch.is_tensor(seg_mask):
        raise ValueError("seg_filter needs seg_mask: the int64 [N, H, W] arg-max class map (or the [N, C, H, W] seg logits) as a tensor")
    W, H = int(codec.input_width), int(codec.input_height)
    if seg_mask.dim() == 4:
        ok = seg_mask.is_floating_point() and (seg_mask.shape[0], seg_mask.shape[2], seg_mask.shape[3]) == (n, H, W)
    else:
        ok = seg_mask.dim() == 3 and seg_mask.dtype == torch.int64 and tuple(seg_mask.shape) == (n, H, W)
    if not ok:
        raise ValueError("seg_mask is the int64 [%d, %d, %d] class map of the net input size or float [%d, C, %d, %d] logits, not %s %s"
                         % (n, H, W, n, H, W, seg_mask.dtype, tuple(seg_mask.shape)))
    interval = float(codec.interval)
    if not (interval.is_integer() and interval >= 1):
        raise ValueError("the seg filter paints on integer rows: the codec's interval %r is not a whole number of pixels" % codec.interval)
    if H % int(codec.step_w) or W % int(codec.step_w):
        raise ValueError("the seg filter needs an input size that is a multiple of the anchor stride, not %dx%d / %d" % (W, H, codec.step_w))
    return int(interval)


def _launch_seg_filter(X, ints, counts, n, W, H, stride, ppl, interval, seg_mask, f):
    """hn_lane_seg_filter behind hn_lane_decode_nms on the same stream: ints [5, n, hw] holds start, end, order, keep and takes keep_out
    as its fifth plane -> the int32 tensor stats [n, top_k, 4] ++ n_sel [n]"""
    dev = X.device
    seg_mask = seg_mask.to(dev)
    if seg_mask.dim() == 4:
        from . import ops as K
        seg_mask = K.argmax_channels(seg_mask.detach().float())
    seg_mask = seg_mask.contiguous()
    need = lib().query("hn_lane_seg_filter_ws_bytes", n, f.top_k, ppl)
    if need < 0:
        raise ValueError("the seg filter holds 1 .. 1024 points per line and 1 .. 65535 images, not %d and %d" % (ppl, n))
    ws = torch.empty((need,), device=dev, dtype=torch.uint8)
    ext = torch.empty((n * f.top_k * 4 + n,), device=dev, dtype=torch.int32)
    lib().call("hn_lane_seg_filter", X.data_ptr(), ints[0].data_ptr(), ints[1].data_ptr(), ints[2].data_ptr(), ints[3].data_ptr(),
               counts.data_ptr(), n, W, H, stride, ppl, interval, seg_mask.data_ptr(), int(f.lane_class), int(f.line_width), float(f.min_ratio),
               int(f.top_k), ws.data_ptr(), need, ints[4].data_ptr(), ext.data_ptr(), ext.data_ptr() + 4 * n * f.top_k * 4)
    return ext


def _decode_batch(cls, loc, codec, conf_thres, nms_thres, use_mean, margin=100.0, keep_all=False, seg_mask=None, seg_filter=None,
                  return_stats=False):
    assert getattr(codec, "scale_invariance", True), "only the scale-invariant location encoding of the shipped cfgs is on the device path"
    interval = _check_seg_filter(seg_mask, seg_filter, return_stats, codec, cls.shape[0])
    dev = cls.device if cls.is_cuda else torch.device("cuda", torch.cuda.current_device())
    cls = cls.detach().to(dev, torch.float32).contiguous()
    loc = loc.detach().to(dev, torch.float32).contiguous()
    n, hw, _ = cls.shape
    W, H, stride, ppl = int(codec.input_width), int(codec.input_height), int(codec.step_w), int(codec.points_per_line)
    assert hw == (W // stride) * (H // stride) and loc.shape == (n, hw, 2 * ppl + 2), (cls.shape, loc.shape)
    X = torch.empty((n, hw, ppl), device=dev, dtype=torch.float32)
    prob = torch.empty((n, hw), device=dev, dtype=torch.float32)
    ints = torch.empty((4 if seg_filter is None else 5, n, hw), device=dev, dtype=torch.int32)
    counts = torch.empty((n,), device=dev, dtype=torch.int32)
    lib().call("hn_lane_decode_nms", cls.data_ptr(), loc.data_ptr(), n, W, H, stride, ppl, float(conf_thres), float(nms_thres), 1 if use_mean else 0,
               float(margin), X.data_ptr(), prob.data_ptr(), ints[0].data_ptr(), ints[1].data_ptr(), ints[2].data_ptr(), ints[3].data_ptr(),
               counts.data_ptr())
    if seg_filter is not None:             # the filter's launches follow on the same stream; its outputs come back with the decode's arrays
        ext = _launch_seg_filter(X, ints, counts, n, W, H, stride, ppl, interval, seg_mask, seg_filter)
    counts, prob, ints, X = counts.cpu().numpy(), prob.cpu().numpy(), ints.cpu().numpy(), X.cpu().numpy()
    start, end, order, keep = ints[:4]
    stats = None
    if seg_filter is not None:
        ext = ext.cpu().numpy()
        keep = ints[4]                     # keep_out: the NMS survivors minus the capped and the dropped
        tk = seg_filter.top_k
        rows, n_sel = ext[:n * tk * 4].reshape(n, tk, 4), ext[n * tk * 4:]
        stats = [[{"score": float(prob[i, order[i, j]]), "area": int(ar), "overlap": int(ov), "kept": bool(kp)}
                  for j, ar, ov, kp in rows[i, :int(n_sel[i])].tolist()] for i in range(n)]
    fw = W // stride
    out = []
    for i in range(n):
        lanes = []
        for j in range(int(counts[i])):
            if not (keep_all or keep[i, j]):
                continue
            a = int(order[i, j])
            s, e = int(start[i, a]), int(end[i, a])
            pts = np.array([Point(X[i, a, p], H - 1 - p * codec.interval) for p in range(s, e)])
            ah, aw = divmod(a, fw)
            lanes.append(Lane(prob[i, a], s, e, (1.0 * aw + 0.5) * stride, (1.0 * ah + 0.5) * stride, 1, pts))
        if keep_all:                       # decode_lane returns raster order
            lanes.sort(key=lambda l: (l.ay, l.ax))
        out.append(lanes)
    return (out, stats) if return_stats else out


def decode(predict_cls, predict_loc, pointlane, conf_thres=0.5, nms_line_thres=100, use_mean=False, seg_mask=None, seg_filter=None,
           return_stats=False):
    """LaneHeader.decode (lanedetect.py:103-116) for ONE image: predict_cls [hw, 2] logits, predict_loc [hw, 2*ppl+2].  seg_filter (a
    LaneSegFilter) with seg_mask (the image's int64 [H, W] arg-max class map or its [C, H, W] seg logits): the deploy path's cap and
    marking-class filter on the device, see decode_batch; return_stats: (lanes, stats of the selected lanes)."""
    if seg_mask is not None and torch.is_tensor(seg_mask):
        seg_mask = seg_mask[None]
    r = _decode_batch(predict_cls[None], predict_loc[None], pointlane, conf_thres, nms_line_thres, use_mean, seg_mask=seg_mask,
                      seg_filter=seg_filter, return_stats=return_stats)
    return (r[0][0], r[1][0]) if return_stats else r[0]


def decode_batch(predict_cls, predict_loc, pointlane, conf_thres=0.5, nms_line_thres=100, use_mean=False, seg_mask=None, seg_filter=None,
                 return_stats=False):
    """the same for a whole batch [N, hw, 2] / [N, hw, L] in one launch.  With seg_filter (a LaneSegFilter) and seg_mask (the int64
    [N, H, W] arg-max class map of the net input size, or the [N, C, H, W] seg logits, reduced by argmax_channels) the lanes the NMS leaves
    are capped and filtered by the seg head's marking class on the device (hn_lane_seg_filter) before the one readback, and
    only the survivors are returned; return_stats: (lanes, stats), stats[i] = one {"score", "area", "overlap", "kept"} per selected lane of
    image i in descending-score order.  Without seg_filter nothing is launched or returned beyond the decode."""
    return _decode_batch(predict_cls, predict_loc, pointlane, conf_thres, nms_line_thres, use_mean, seg_mask=seg_mask, seg_filter=seg_filter,
                         return_stats=return_stats)


# ---- host-side bookkeeping on the surviving lanes (lane_codec_utils.py:66-124,185-282) ----------------------------------------------
def _calc_y_cross(p1, p2, y):
    if abs(p1.y - p2.y) < 1e-6:
        return -1
    k = (p1.x - p2.x) / (p1.y - p2.y)
    return k * y + (p1.x - k * p1.y)


class _LaneWithCrossK:
    def __init__(self, lane_, idx_in, y_in):
        self.lane, self.idx, self.y = lane_, idx_in, y_in
        pts = lane_.lane
        if pts[1].y < pts[0].y:
            self.k = (pts[1].x - pts[0].x) / (pts[1].y - pts[0].y)
            self.cross_x = _calc_y_cross(pts[0], pts[1], y_in)
        elif pts[1].y > pts[0].y:
            self.k = (pts[-1].x - pts[-2].x) / (pts[-1].y - pts[-2].y)
            self.cross_x = _calc_y_cross(pts[-2], pts[-1], y_in)
        else:
            self.k = 1000
            self.cross_x = _calc_y_cross(pts[-2], pts[-1], y_in)

    def __lt__(self, other):
        if abs(self.cross_x - other.cross_x) > 2.0:
            return self.cross_x < other.cross_x
        if self.lane.lane[1].y < self.lane.lane[0].y:
            return self.lane.lane[-1].x < other.lane.lane[-1].x
        return self.lane.lane[0].x < other.lane.lane[0].x


def order_lane_x_axis(lane_set, h):
    if len(lane_set) == 0:
        return list()
    srt = sorted(_LaneWithCrossK(l, i, h - 1.0) for i, l in enumerate(lane_set))
    right = len(srt)
    for i, l in enumerate(srt):
        if l.k > 0:
            right = i
            break
    idx = [None] * len(srt)
    for j, i in enumerate(range(right - 1, -1, -1)):
        idx[i] = -1 - j
    for j, i in enumerate(range(right, len(srt))):
        idx[i] = 1 + j
    out = []
    for i, l in enumerate(srt):
        l.lane.idx = idx[i]
        out.append(l.lane)
    return out


def convert_lane_to_dict(lane_set, sx, sy):
    lines = []
    for l in lane_set:
        if l.prob < 0.01:
            continue
        lines.append({"score": l.prob, "points": [{"x": p.x * sx, "y": p.y * sy} for p in l.lane]})
    return {"Lines": lines}


def scale_to_org(lane_nms_set, net_input_width, net_input_height, org_width, org_height):
    """LaneHeader.scale_to_org, lanedetect.py:118-124"""
    ordered = order_lane_x_axis(list(lane_nms_set), net_input_height)
    return convert_lane_to_dict(ordered, org_width / net_input_width, org_height / net_input_height)
