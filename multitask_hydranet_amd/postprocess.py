"""Detection post-processing on the device (head_detect/detection_loss.py:7-108 of the reference: BBoxTransform, ClipBoxes, postprocess).

One HIP pipeline for the whole batch (hn_det_postprocess, csrc/hn_post.hip): box decode + clip + per-anchor max / arg-max class + score
threshold compaction + stable descending-score order + class-offset greedy NMS + gather.  No per-image host loop, no host NMS: the only
device-to-host traffic is the final result (kept boxes, classes, scores and two counters per image), which the reference's contract returns
as numpy arrays.  Index bookkeeping is exact; torchvision.ops.batched_nms (unpinned third party in the reference, absent here) is restated
from its published semantics -- stable descending score order, suppress when IoU > threshold, IoU = inter / (a + b - inter), classes
separated by an offset of class_id * (max kept coordinate + 1) -- see DESIGN.md ("parity unpinned for NMS").
NmsOptions makes the suppression rule an option (hn_det_postprocess_ex: DIoU-NMS, Soft-NMS, max_det, class-agnostic); without
one every call is the one above.
There is no CPU path: CPU tensors are moved to the current HIP device first; without the HIP library this module raises.
"""
from __future__ import annotations

import math
from typing import Optional

import numpy as np
import torch

from ._lib import lib

MAX_CAP = 32768
NMS_KINDS = ("hard", "diou", "soft_linear", "soft_gaussian")          # index = nms_kind of hn_det_postprocess_ex


class NmsOptions:
    """The suppression rule of the detection post-process (hn_det_postprocess_ex).
    kind: "hard" (greedy, suppress when IoU > iou_threshold), "diou" (the same walk on IoU - rho^2 / c^2), "soft_linear" / "soft_gaussian"
    (Soft-NMS: the winner decays the other scores by 1 - IoU when IoU > iou_threshold, or by exp(-IoU^2 / sigma); the scores returned are
    the decayed ones).  score_floor: a decayed box leaves when its score is no longer above it (None: the call's score threshold).
    max_det: at most that many boxes per image (0: no limit).  class_agnostic: boxes of different classes suppress each other."""

    __slots__ = ("kind", "sigma", "score_floor", "max_det", "class_agnostic")

    def __init__(self, kind="hard", sigma=0.5, score_floor=None, max_det=0, class_agnostic=False):
        if kind not in NMS_KINDS:
            raise ValueError("NmsOptions.kind must be one of %s, got %r" % (", ".join(repr(k) for k in NMS_KINDS), kind))
        if isinstance(sigma, bool) or not isinstance(sigma, (int, float)) or not math.isfinite(sigma) or not sigma > 0:
            raise ValueError("NmsOptions.sigma must be a finite number > 0, got %r" % (sigma,))
        if score_floor is not None and (isinstance(score_floor, bool) or not isinstance(score_floor, (int, float)) or math.isnan(score_floor)):
            raise ValueError("NmsOptions.score_floor must be a number or None, got %r" % (score_floor,))
        if isinstance(max_det, bool) or not isinstance(max_det, int) or max_det < 0:
            raise ValueError("NmsOptions.max_det must be an integer >= 0 (0: no limit), got %r" % (max_det,))
        self.kind, self.sigma, self.max_det, self.class_agnostic = kind, float(sigma), int(max_det), bool(class_agnostic)
        self.score_floor = None if score_floor is None else float(score_floor)

    def __repr__(self):
        return "NmsOptions(kind=%r, sigma=%r, score_floor=%r, max_det=%r, class_agnostic=%r)" % (
            self.kind, self.sigma, self.score_floor, self.max_det, self.class_agnostic)

    def __eq__(self, other):
        return isinstance(other, NmsOptions) and all(getattr(self, k) == getattr(other, k) for k in self.__slots__)

    def __hash__(self):
        return hash(tuple(getattr(self, k) for k in self.__slots__))


def decode_boxes(anchors: torch.Tensor, regression: torch.Tensor) -> torch.Tensor:
    """BBoxTransform.forward (detection_loss.py:7-33) as tensor ops, kept for callers that want the raw decoded boxes"""
    yca = (anchors[..., 0] + anchors[..., 2]) / 2
    xca = (anchors[..., 1] + anchors[..., 3]) / 2
    ha = anchors[..., 2] - anchors[..., 0]
    wa = anchors[..., 3] - anchors[..., 1]
    w = regression[..., 3].exp() * wa
    h = regression[..., 2].exp() * ha
    yc = regression[..., 0] * ha + yca
    xc = regression[..., 1] * wa + xca
    return torch.stack([xc - w / 2.0, yc - h / 2.0, xc + w / 2.0, yc + h / 2.0], dim=2)


def postprocess_device(img_hw, anchors, regression, classification, threshold, iou_threshold, cap: int = 4096, nms: Optional[NmsOptions] = None):
    """device tensors in, device tensors out: dict(rois [N,cap,4], class_ids [N,cap] int64, scores [N,cap], kept [N] int32, total [N] int32).
    Row i < kept[n] of image n is its i-th detection in descending score order.  total[n] > cap means image n overflowed the capacity.
    nms: the suppression rule (NmsOptions; hn_det_postprocess_ex); None is hn_det_postprocess, the reference's hard NMS."""
    if nms is not None and not isinstance(nms, NmsOptions):
        raise ValueError("nms is an NmsOptions or None, not %r" % (nms,))
    h, w = img_hw
    dev = regression.device if regression.is_cuda else torch.device("cuda", torch.cuda.current_device())
    reg = regression.detach().to(dev, torch.float32).contiguous()
    cls = classification.detach().to(dev, torch.float32).contiguous()
    anc = anchors.detach().to(dev, torch.float32)
    anc = (anc[0] if anc.dim() == 3 else anc).contiguous()
    n, a, k = cls.shape
    assert reg.shape == (n, a, 4) and anc.shape == (a, 4), (reg.shape, anc.shape)
    cap = int(min(max(cap, 1), MAX_CAP, a))
    kind = 0 if nms is None else NMS_KINDS.index(nms.kind)
    ws_bytes = lib().query("hn_det_post_ws_bytes", n, cap) if nms is None else lib().query("hn_det_post_ws_bytes_ex", n, cap, kind)
    ws = torch.empty((ws_bytes,), device=dev, dtype=torch.uint8)
    out = dict(rois=torch.empty((n, cap, 4), device=dev, dtype=torch.float32), class_ids=torch.empty((n, cap), device=dev, dtype=torch.int64),
               scores=torch.empty((n, cap), device=dev, dtype=torch.float32), kept=torch.empty((n,), device=dev, dtype=torch.int32),
               total=torch.empty((n,), device=dev, dtype=torch.int32))
    args = (anc.data_ptr(), reg.data_ptr(), cls.data_ptr(), n, a, k, int(h), int(w), float(threshold), float(iou_threshold), cap, ws.data_ptr(),
            out["rois"].data_ptr(), out["class_ids"].data_ptr(), out["scores"].data_ptr(), out["kept"].data_ptr(), out["total"].data_ptr())
    if nms is None:
        lib().call("hn_det_postprocess", *args)
    else:
        floor = float(threshold) if nms.score_floor is None else nms.score_floor
        lib().call("hn_det_postprocess_ex", *args, kind, nms.sigma, floor, nms.max_det, int(nms.class_agnostic))
    out["cap"] = cap
    return out


def postprocess(img_hw, anchors, regression, classification, threshold, iou_threshold, nms: Optional[NmsOptions] = None, launched=None):
    """the reference's return contract: one dict(rois, class_ids, scores) of numpy arrays per image (empty arrays when nothing is kept).
    launched: what postprocess_device returned for the same arguments at the default capacity, when the caller has launched it already
    (to read its result back at a synchronisation point of its own choosing).  nms: see postprocess_device; the retries after a capacity
    overflow run with it too."""
    cap = 4096
    while True:
        res = launched if launched is not None else postprocess_device(img_hw, anchors, regression, classification, threshold, iou_threshold, cap,
                                                                           nms)
        launched = None
        total = res["total"].cpu().numpy()
        if int(total.max(initial=0)) <= res["cap"]:
            break
        if res["cap"] >= min(MAX_CAP, regression.shape[1]):
            raise RuntimeError(f"{int(total.max())} anchors over the score threshold in one image: the device NMS holds at most {MAX_CAP}")
        cap = min(MAX_CAP, max(2 * cap, int(total.max())))
    kept = res["kept"].cpu().numpy()
    rois, cids, scores = res["rois"].cpu().numpy(), res["class_ids"].cpu().numpy(), res["scores"].cpu().numpy()
    out = []
    for i in range(len(kept)):
        k = int(kept[i])
        if k == 0:
            out.append(dict(rois=np.array(()), class_ids=np.array(()), scores=np.array(())))
        else:
            out.append(dict(rois=rois[i, :k].copy(), class_ids=cids[i, :k].copy(), scores=scores[i, :k].copy()))
    return out
