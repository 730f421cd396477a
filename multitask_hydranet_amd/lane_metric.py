"""Lane F1 for validation (reference: head_lane/lane_metric.py:166-440, driven by train.py:188,380-397,433).

`LaneMetric(method="f1_measure", iou_thresh=0.5, lane_width=30, thresh_list=[0.5])` keeps the reference's interface: call it with
`output=[dict(pr_result={"Lines": [...], "Shape": {...}}, gt_result={"Lines": [...], "Labels": [...], "Shape": {...}}), ...]`, then
`summary()`.  Per image: every lane is a natural cubic spline through its points, sampled at unit arc steps (spline_interp, restated with
the reference's arithmetic incl. its 1e-8 guards), drawn with width `lane_width` into a mask of the source-image size; IoU matrix of ground
truth x prediction masks; Hungarian assignment (scipy, as the reference); a matched pair with IoU > iou_thresh is a hit; precision / recall /
F1 over the epoch.  The rasterisation and the pixel counts run on the device (hn_lane_raster, hn_lane_iou: one launch each per image, exact
integer counts); the 1080 x 1920 masks never leave HBM.  cv2.line is restated (pixels within lane_width / 2 of the segment): parity with
OpenCV's thick-line fill at boundary pixels is unpinned (cv2 is absent), everything else is pinned by tests/golden/lane_metric.json.
`LaneMetric(..., batched=True)` gives the same records from one launch sequence per call and one synchronisation per summary (LaneIoUBatch,
hn_lane_metric.hip: spline, samples, rasterisation and counts of a ragged batch on the device; pinned by tests/golden/lane_metric_batch.json)."""
from __future__ import annotations

import sys
from typing import Dict, List, Sequence

import numpy as np
import torch

from ._lib import lib


def calc_params(lane: Sequence[dict]) -> List[dict]:
    """natural cubic spline over the chord-length parameter, one segment record per point pair (lane_metric.py:71-146)"""
    n = len(lane)
    if n < 2:
        return []
    xs = [p["x"] for p in lane]
    ys = [p["y"] for p in lane]
    if n == 2:
        h0 = np.sqrt((xs[0] - xs[1]) * (xs[0] - xs[1]) + (ys[0] - ys[1]) * (ys[0] - ys[1]))
        return [dict(a_x=xs[0], b_x=(xs[1] - xs[0]) / (h0 + 1e-8), c_x=0, d_x=0, a_y=ys[0], b_y=(ys[1] - ys[0]) / (h0 + 1e-8), c_y=0, d_y=0, h=h0)]
    h = [np.sqrt((xs[i] - xs[i + 1]) * (xs[i] - xs[i + 1]) + (ys[i] - ys[i + 1]) * (ys[i] - ys[i + 1])) for i in range(n - 1)]
    # Thomas sweep of the tridiagonal system for the second derivatives M_1 .. M_{n-2} (M_0 = M_{n-1} = 0)
    cs, dxs, dys = [], [], []
    for i in range(n - 2):
        a, b, c = h[i], 2 * (h[i] + h[i + 1]), h[i + 1]
        tx = 6 * ((xs[i + 2] - xs[i + 1]) / (h[i + 1] + 1e-8) - (xs[i + 1] - xs[i]) / (h[i] + 1e-8))
        ty = 6 * ((ys[i + 2] - ys[i + 1]) / (h[i + 1] + 1e-8) - (ys[i + 1] - ys[i]) / (h[i] + 1e-8))
        if i == 0:
            cs.append(c / (b + 1e-8))
            dxs.append(tx / (b + 1e-8))
            dys.append(ty / (b + 1e-8))
        else:
            base = b - a * cs[i - 1]
            cs.append(c / (base + 1e-8))
            dxs.append((tx - a * dxs[i - 1]) / (base + 1e-8))
            dys.append((ty - a * dys[i - 1]) / (base + 1e-8))
    mx, my = np.zeros(n), np.zeros(n)
    mx[n - 2], my[n - 2] = dxs[n - 3], dys[n - 3]
    for i in range(n - 4, -1, -1):
        mx[i + 1] = dxs[i] - cs[i] * mx[i + 2]
        my[i + 1] = dys[i] - cs[i] * my[i + 2]
    mx[0] = mx[-1] = my[0] = my[-1] = 0
    out = []
    for i in range(n - 1):
        out.append(dict(a_x=xs[i], b_x=(xs[i + 1] - xs[i]) / (h[i] + 1e-8) - (2 * h[i] * mx[i] + h[i] * mx[i + 1]) / 6, c_x=mx[i] / 2,
                        d_x=(mx[i + 1] - mx[i]) / (6 * (h[i] + 1e-8)),
                        a_y=ys[i], b_y=(ys[i + 1] - ys[i]) / (h[i] + 1e-8) - (2 * h[i] * my[i] + h[i] * my[i + 1]) / 6, c_y=my[i] / 2,
                        d_y=(my[i + 1] - my[i]) / (6 * (h[i] + 1e-8)), h=h[i]))
    return out


def spline_interp(*, lane: Sequence[dict], step_t=1) -> List[dict]:
    """lane_metric.py:45-68: samples of the spline at t = 0, step_t, ... < h per segment, then the last point"""
    if len(lane) < 2:
        return list(lane)
    pts = []
    for f in calc_params(lane):
        t = 0
        while t < f["h"]:
            pts.append({"x": f["a_x"] + f["b_x"] * t + f["c_x"] * t * t + f["d_x"] * t * t * t,
                        "y": f["a_y"] + f["b_y"] * t + f["c_y"] * t * t + f["d_y"] * t * t * t})
            t += step_t
    pts.append(lane[-1])
    return pts


def iou_matrix(gt_lanes: Sequence[Sequence[dict]], pr_lanes: Sequence[Sequence[dict]], height: int, width: int, lane_width: int,
               device=None) -> np.ndarray:
    """calc_iou (lane_metric.py:166-209) for every (ground truth, prediction) pair of one image, on the device.  Any number of lanes (the
    reference has no limit; a noisy early-epoch decode can keep more than the pair kernel's 32 x 32 block: it then runs per block)"""
    g, p = len(gt_lanes), len(pr_lanes)
    assert g > 0 and p > 0, (g, p)
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    pts, seg_lane, seg_first = [], [], []
    for li, lane in enumerate(list(gt_lanes) + list(pr_lanes)):
        ip = spline_interp(lane=lane, step_t=1)
        base = len(pts)
        pts += [(int(q["x"]), int(q["y"])) for q in ip]                     # int(): truncation toward zero, as the reference's cv2.line arguments
        for i in range(len(ip) - 1):
            seg_lane.append(li)
            seg_first.append(base + i)
    masks = torch.zeros((g + p, height, width), dtype=torch.uint8, device=dev)
    if seg_lane:
        tp = torch.tensor(pts, dtype=torch.int32).to(dev)
        tl, tf = torch.tensor(seg_lane, dtype=torch.int32).to(dev), torch.tensor(seg_first, dtype=torch.int32).to(dev)
        lib().call("hn_lane_raster", tp.data_ptr(), tl.data_ptr(), tf.data_ptr(), len(seg_lane), int(lane_width), height, width, masks.data_ptr())
    B = 32                                                                  # hn_lane_iou's pair block (bit masks per pixel)
    if g <= B and p <= B:
        inter = torch.zeros((g, p), dtype=torch.int64, device=dev)
        area = torch.zeros((g + p,), dtype=torch.int64, device=dev)
        lib().call("hn_lane_iou", masks.data_ptr(), g, p, height * width, inter.data_ptr(), area.data_ptr())
    else:
        inter = torch.zeros((g, p), dtype=torch.int64, device=dev)
        area = torch.zeros((g + p,), dtype=torch.int64, device=dev)
        for g0 in range(0, g, B):
            for p0 in range(0, p, B):
                gc, pc = min(B, g - g0), min(B, p - p0)
                sub = torch.cat([masks[g0:g0 + gc], masks[g + p0:g + p0 + pc]]).contiguous()
                bi = torch.zeros((gc, pc), dtype=torch.int64, device=dev)
                ba = torch.zeros((gc + pc,), dtype=torch.int64, device=dev)
                lib().call("hn_lane_iou", sub.data_ptr(), gc, pc, height * width, bi.data_ptr(), ba.data_ptr())
                inter[g0:g0 + gc, p0:p0 + pc] = bi
                area[g0:g0 + gc] = ba[:gc]
                area[g + p0:g + p0 + pc] = ba[gc:]
    inter, area = inter.cpu().numpy().astype(np.float64), area.cpu().numpy().astype(np.float64)
    union = area[:g, None] + area[None, g:] - inter
    # (the reference sums uint8 masks of value 255: the factor cancels in the ratio; an empty union scores 0)
    return np.where(union > 0, inter / np.maximum(union, 1.0), 0.0)


def evaluate_core(*, gt_lanes, pr_lanes, gt_wh, pr_wh, hyperp) -> Dict[str, int]:
    """lane_metric.py:215-272: Hungarian assignment on 1 - IoU, hits = matched pairs with IoU > iou_thresh"""
    from scipy.optimize import linear_sum_assignment
    gt_num, pr_num, hit = len(gt_lanes), len(pr_lanes), 0
    if gt_num > 0 and pr_num > 0:
        iou = iou_matrix(gt_lanes, pr_lanes, hyperp["eval_height"], hyperp["eval_width"], hyperp["lane_width"])
        for gi, pi in zip(*linear_sum_assignment(1 - iou)):
            if iou[gi][pi] > hyperp["iou_thresh"]:
                hit += 1
    return dict(gt_num=gt_num, pr_num=pr_num, hit_num=hit)


class LaneMetricCore:
    """lane_metric.py:311-389"""

    def __init__(self, *, iou_thresh, lane_width, prob_thresh=None):
        self.eval_params = dict(iou_thresh=iou_thresh, lane_width=lane_width)
        self.prob_thresh = prob_thresh
        self.result_record: List[dict] = []

    def __call__(self, gt_result, pr_result, *args, **kwargs):
        gt_wh, pr_wh = gt_result["Shape"], pr_result["Shape"]
        gt_lanes = [line for line, _ in zip(gt_result["Lines"], gt_result["Labels"]) if len(line) > 0]
        pr_lanes = []
        for line in pr_result["Lines"]:
            if "score" in line:
                line = line["points"] if line["score"] > self.prob_thresh else []
            if len(line) > 0:
                pr_lanes.append(line)
        self.eval_params["eval_width"], self.eval_params["eval_height"] = gt_wh["width"], gt_wh["height"]
        self.result_record.append(evaluate_core(gt_lanes=gt_lanes, pr_lanes=pr_lanes, gt_wh=gt_wh, pr_wh=pr_wh, hyperp=self.eval_params))

    def reset(self):
        self.result_record = []

    def summary(self):
        hit = sum(r["hit_num"] for r in self.result_record)
        pr = sum(r["pr_num"] for r in self.result_record)
        gt = sum(r["gt_num"] for r in self.result_record)
        precision = hit / (pr + sys.float_info.epsilon)
        recall = hit / (gt + sys.float_info.epsilon)
        return dict(f1_measure=2 * precision * recall / (precision + recall + sys.float_info.epsilon), precision=precision, recall=recall)


class LaneMetric:
    """lane_metric.py:392-440.  batched=True: the same records and summaries from LaneIoUBatch (below): every image is added once with all
    of its predictions, the device work of a call is enqueued without a host synchronisation, and the first read of a handler's
    result_record / summary() synchronises once and scores every threshold on the host from the count tables (the IoU matrix of the
    predictions above a threshold is a sub-matrix of the image's)."""

    def __init__(self, *, method, iou_thresh, lane_width, thresh_list=None, batched=False, device=None):
        if method not in ("f1_measure", "precision", "recall"):
            raise NotImplementedError("method should be one of ['f1_measure', 'precision', 'recall']")
        self.method = method
        self.eval_params = dict(iou_thresh=iou_thresh, lane_width=lane_width)
        self.batched = batched
        core = (lambda **kw: _BatchedCore(self, **kw)) if batched else LaneMetricCore
        self.metric_handlers = [core(**self.eval_params, prob_thresh=t) for t in thresh_list] if thresh_list is not None \
            else [core(**self.eval_params, prob_thresh=None)]
        if batched:
            self._batch = LaneIoUBatch(lane_width, device=device)
            self._pending = []                                              # (image index, scores of its predictions) not yet scored

    def __call__(self, output, *args, **kwargs):
        if self.batched:
            for pair in output:
                gt, pr = pair["gt_result"], pair["pr_result"]
                gt_lanes = [line for line, _ in zip(gt["Lines"], gt["Labels"]) if len(line) > 0]
                pr_lanes, scores = [], []
                for line in pr["Lines"]:
                    score = None
                    if "score" in line:
                        score, line = line["score"], line["points"]
                    if len(line) > 0:
                        pr_lanes.append(line)
                        scores.append(score)
                self._pending.append((self._batch.add(gt_lanes, pr_lanes, gt["Shape"]["height"], gt["Shape"]["width"]), scores))
            self._batch.flush()
            return
        for handler in self.metric_handlers:
            for pair in output:
                handler(**pair)

    def _drain(self):
        """the one synchronisation: score what has been added since the last one, for every handler"""
        if not self._pending:
            return
        from scipy.optimize import linear_sum_assignment
        res = self._batch.result()
        for idx, scores in self._pending:
            iou = res[idx]["iou"]
            for h in self.metric_handlers:
                keep = [i for i, s in enumerate(scores) if s is None or s > h.prob_thresh]
                hit = 0
                if iou.shape[0] > 0 and keep:
                    sub = iou[:, keep]
                    for gi, pi in zip(*linear_sum_assignment(1 - sub)):
                        if sub[gi][pi] > h.eval_params["iou_thresh"]:
                            hit += 1
                h._records.append(dict(gt_num=iou.shape[0], pr_num=len(keep), hit_num=hit))
        self._pending = []
        self._batch = LaneIoUBatch(self.eval_params["lane_width"], device=self._batch.device)

    def reset(self):
        for handler in self.metric_handlers:
            handler.reset()

    def summary(self):
        return max(h.summary()[self.method] for h in self.metric_handlers)


class _BatchedCore(LaneMetricCore):
    """a handler of LaneMetric(batched=True): result_record, summary() and reset() as LaneMetricCore's, filled by the owner's _drain()"""

    def __init__(self, owner, **kw):
        self._owner = owner
        self._records: List[dict] = []
        super().__init__(**kw)

    @property
    def result_record(self):
        self._owner._drain()
        return self._records

    @result_record.setter
    def result_record(self, value):
        self._records = value

    def __call__(self, gt_result, pr_result, *args, **kwargs):
        raise TypeError("a handler of LaneMetric(batched=True) is fed through LaneMetric.__call__")

    def reset(self):
        if hasattr(self._owner, "_pending"):
            self._owner._drain()                                            # what has been handed in so far is scored, then dropped
        self._records = []


# --------------------------------------------------------------------------------------------------------------------------------------
# the same IoU matrices for a ragged batch of images at once (hn_lane_metric.hip)
# --------------------------------------------------------------------------------------------------------------------------------------
LANE_TILE = 64                  # pixels per side of a workgroup's tile
LANE_BLOCK = 32                 # lanes per side of a pair block
MAX_SAMPLES = 1 << 26           # per batch (a 1080p lane has about a thousand)


def pack_lane_batch(items):
    """items: [(gt_lanes, pr_lanes, height, width)], a lane = [{"x":, "y":}, ...] -> (pts float64 [n_points][2], tab int32, meta): the
    tables of hn_lane_metric_batch (include/hydranet_hip.h) and meta = dict(N, n_lanes, n_points, n_work, n_tiles, sample_cap, n_counts,
    images=[(G, P, cnt_off)], and the views lane_off / img_lane / img_g / img_h / img_w / cnt_off / work into tab).  sample_cap is the
    batch's exact number of samples: the chord lengths are numpy's here and on the device (correctly rounded), and segment i has as many
    samples as `t = 0; while t < h_i: t += 1` has turns."""
    n = len(items)
    xy, lane_off, img_lane, img_g, img_h, img_w, cnt_off, work, images = [], [0], [0], [], [], [], [], [], []
    n_counts = n_tiles = 0
    for b, (gts, prs, height, width) in enumerate(items):
        height, width = int(height), int(width)
        if height <= 0 or width <= 0 or height > 65536 or width > 65536:
            raise ValueError(f"image {b}: evaluation size {height} x {width}")
        for lane in list(gts) + list(prs):
            xy += [(float(p["x"]), float(p["y"])) for p in lane]
            lane_off.append(len(xy))
        g, p = len(gts), len(prs)
        img_lane.append(len(lane_off) - 1)
        img_g.append(g)
        img_h.append(height)
        img_w.append(width)
        cnt_off.append(n_counts)
        images.append((g, p, n_counts))
        n_counts += g * p + g + p
        tiles = -(-height // LANE_TILE) * -(-width // LANE_TILE)
        if g + p > 0:
            for g0 in range(0, max(g, 1), LANE_BLOCK):
                for p0 in range(0, max(p, 1), LANE_BLOCK):
                    work.append((b, g0, p0, n_tiles))
                    n_tiles += tiles
    pts = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    if not np.isfinite(pts).all():
        raise ValueError("a lane point is not finite")
    lane_off = np.asarray(lane_off, dtype=np.int64)
    cap = 0
    if len(pts):
        d = pts[:-1] - pts[1:]
        h = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])                  # (the entries across two lanes are dropped below)
        last = np.zeros(len(pts), dtype=bool)
        last[lane_off[1:][lane_off[1:] > lane_off[:-1]] - 1] = True         # every non-empty lane's last point: one sample
        seg = ~last[:-1]
        if seg.any() and float(h[seg].max()) >= 1e9:
            raise ValueError("a lane segment is longer than 1e9 pixels")
        cap = int(np.where(h[seg] > 0, np.ceil(h[seg]), 0).sum()) + int(last.sum())
    n_counts += 1                                                           # the status word
    if cap > MAX_SAMPLES or n_counts >= 2 ** 31 or n_tiles >= 2 ** 31:
        raise ValueError(f"lane batch too large: {cap} samples, {n_counts} counts, {n_tiles} tiles")
    parts = [lane_off, img_lane, img_g, img_h, img_w, cnt_off, np.asarray(work, dtype=np.int64).reshape(-1)]
    tab = np.concatenate([np.asarray(a, dtype=np.int64) for a in parts]).astype(np.int32)
    meta = dict(N=n, n_lanes=len(lane_off) - 1, n_points=len(pts), n_work=len(work), n_tiles=n_tiles, sample_cap=cap, n_counts=n_counts, images=images)
    o = 0
    for name, a in zip(("lane_off", "img_lane", "img_g", "img_h", "img_w", "cnt_off", "work"), parts):
        meta[name] = tab[o:o + len(a)]
        o += len(a)
    meta["work"] = meta["work"].reshape(-1, 4)
    return pts, tab, meta


def iou_from_counts(table: np.ndarray, g: int, p: int) -> np.ndarray:
    """an image's count table (|g & p| [G][P], |g| [G], |p| [P]) -> the float64 IoU matrix [G][P], as iou_matrix"""
    inter = table[:g * p].reshape(g, p).astype(np.float64)
    area = table[g * p:].astype(np.float64)
    union = area[:g, None] + area[None, g:] - inter
    return np.where(union > 0, inter / np.maximum(union, 1.0), 0.0)


class LaneIoUBatch:
    """IoU matrices of many images with one synchronisation.  add() packs an image on the host and returns its index; flush() sends what has
    been added as ONE batch (one host-to-device copy, hn_lane_metric_batch, one copy back into pinned memory) without waiting for it;
    result() waits once and returns, per image added so far, dict(iou=float64 [G][P], inter=int64 [G][P], area_gt=int64 [G], area_pr=int64
    [P]).  keep_samples=True keeps every flush's workspace so that samples() can read the int-truncated spline samples back (tests)."""

    def __init__(self, lane_width, device=None, keep_samples=False):
        self.lane_width = int(lane_width)
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.keep_samples = keep_samples
        self._items = []                                                    # added, not flushed
        self._flushed = []                                                  # (meta, pinned counts, event, workspace or None)
        self._n = 0

    def add(self, gt_lanes, pr_lanes, height, width) -> int:
        self._items.append((list(gt_lanes), list(pr_lanes), height, width))
        self._n += 1
        return self._n - 1

    def flush(self):
        if not self._items:
            return
        pts, tab, m = pack_lane_batch(self._items)
        self._items = []
        pb, tb = pts.size * 8, tab.size * 4
        host = torch.empty(pb + tb, dtype=torch.uint8, pin_memory=True)    # points, then tables: one copy
        hv = host.numpy()
        hv[:pb] = pts.reshape(-1).view(np.uint8)
        hv[pb:] = tab.view(np.uint8)
        with torch.cuda.device(self.device):
            buf = host.to(self.device, non_blocking=True)
            ws_bytes = lib().query("hn_lane_metric_ws_bytes", m["n_lanes"], m["n_points"], m["sample_cap"])
            if ws_bytes < 0:
                raise ValueError(f"lane batch too large: {m['n_points']} points, {m['sample_cap']} samples")
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=self.device)
            counts = torch.empty(m["n_counts"], dtype=torch.int64, device=self.device)
            lib().call("hn_lane_metric_batch", buf.data_ptr(), buf.data_ptr() + pb, m["N"], m["n_lanes"], m["n_points"], m["n_work"], m["n_tiles"],
                       m["sample_cap"], self.lane_width, ws.data_ptr(), ws_bytes, counts.data_ptr(), m["n_counts"])
            out = torch.empty(m["n_counts"], dtype=torch.int64, pin_memory=True)
            out.copy_(counts, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
        self._flushed.append((m, out, ev, ws if self.keep_samples else None))

    def result(self) -> List[dict]:
        self.flush()
        res = []
        for m, out, ev, _ in self._flushed:
            ev.synchronize()                                                # (the first wait that blocks is the only one, on one stream)
            c = out.numpy()
            if c[-1] != 0:
                raise RuntimeError(f"hn_lane_metric_batch: status {int(c[-1])} (more samples than the host's count, or a segment too long)")
            for g, p, o in m["images"]:
                t = c[o:o + g * p + g + p]
                res.append(dict(iou=iou_from_counts(t, g, p), inter=t[:g * p].reshape(g, p).copy(), area_gt=t[g * p:g * p + g].copy(),
                                area_pr=t[g * p + g:].copy()))
        return res

    def samples(self) -> List[List[np.ndarray]]:
        """per image, per lane (ground truths first): the int32 [n][2] (x, y) samples the device painted from.  Needs keep_samples=True."""
        if not self.keep_samples:
            raise RuntimeError("LaneIoUBatch(keep_samples=True) keeps the workspace that holds the samples")
        self.flush()
        res = []
        for m, _, ev, ws in self._flushed:
            ev.synchronize()
            npt = m["n_points"]
            if npt == 0:
                res += [[np.zeros((0, 2), np.int32) for _ in range(m["img_lane"][b + 1] - m["img_lane"][b])] for b in range(m["N"])]
                continue
            raw = ws.cpu().numpy()
            o_off = 14 * 8 * npt
            o_smp = o_off + (4 * (npt + 1) + 15) // 16 * 16 + (4 * npt + 15) // 16 * 16
            off = raw[o_off:o_off + 4 * (npt + 1)].view(np.uint32).astype(np.int64)
            smp = raw[o_smp:o_smp + 16 * m["sample_cap"]].view(np.int32).reshape(-1, 4)
            assert off[-1] == m["sample_cap"], (off[-1], m["sample_cap"])
            for b in range(m["N"]):
                lanes = []
                for l in range(m["img_lane"][b], m["img_lane"][b + 1]):
                    s0, s1 = off[m["lane_off"][l]], off[m["lane_off"][l + 1]]
                    assert (smp[s0:s1, 2] == l).all()
                    lanes.append(smp[s0:s1, :2].copy())
                res.append(lanes)
        return res


def iou_matrices(items, lane_width, device=None) -> List[np.ndarray]:
    """[(gt_lanes, pr_lanes, height, width)] -> every image's float64 IoU matrix [G][P] (iou_matrix's, one batch, one synchronisation; a
    side without lanes gives an empty matrix)"""
    b = LaneIoUBatch(lane_width, device=device)
    for gts, prs, height, width in items:
        b.add(gts, prs, height, width)
    return [r["iou"] for r in b.result()]
