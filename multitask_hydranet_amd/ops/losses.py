"""ops.losses -- segmentation / detection / lane losses, deploy arg-max and the weighted loss sum on HIP kernels (reference:
head_seg/segmentation_loss.py:27-65, head_detect/detection_loss.py:132-267, head_lane/lanedetect_loss.py:18-78, train.py:192-203)."""
from __future__ import annotations

import ctypes
import os
from typing import Optional, Sequence, Tuple

import torch

from .._lib import lib
from .core import *        # noqa: F401,F403
from .backbone import *        # noqa: F401,F403
from .neck import *        # noqa: F401,F403
from .seg import *        # noqa: F401,F403
from .heads import *        # noqa: F401,F403


# --------------------------------------------------------------------------------------------------------------
# Per-image task masks (gt_dict["task_valid"]).  Every loss below takes valid=None: None is the unmasked call; a task's row of
# the mask tensor -- contiguous uint8 [N] on the loss's device, 1 = image n is labelled for the task -- goes to the `_masked` twin of every
# entry point.  The rule: the losses equal the unmasked losses of the sub-batch of labelled images, taken in batch order; without a
# labelled image every loss is 0; the gradient of an unlabelled image's predictions is written as exactly 0.  Same launches as the
# unmasked call, the mask is read on the device, and one captured graph replayed with other mask contents gives those masks' results.
# --------------------------------------------------------------------------------------------------------------
def _task_valid_row(valid, n, dev):
    if (not isinstance(valid, torch.Tensor) or valid.dtype != torch.uint8 or tuple(valid.shape) != (n,) or valid.device != dev
            or not valid.is_contiguous()):
        what = f"{valid.dtype} {tuple(valid.shape)} on {valid.device}" if isinstance(valid, torch.Tensor) else repr(type(valid))
        raise ValueError(f"valid must be a contiguous uint8 [{n}] tensor on {dev}, got {what}")
    return valid


def _masked(name, valid):
    return name if valid is None else name + "_masked"


def _v(valid):
    """the mask argument of a `_masked` entry point (placed before the workspace / outputs), nothing for the unmasked one"""
    return () if valid is None else (ptr(valid),)


# --------------------------------------------------------------------------------------------------------------
# segmentation loss (weighted CE + ignore_index + top-k hardest pixels) and deploy-mode argmax
# --------------------------------------------------------------------------------------------------------------
class SegLoss(torch.autograd.Function):
    """logits: fp32 NHWC [N, H, W, C] (dense rows); target: [N, H, W] int64 or float32 class ids."""

    @staticmethod
    def forward(ctx, logits, target, class_weights, use_top_k, top_k_ratio, ignore_index, slot=None, valid=None):
        """slot (GradSlot of the producing SegOutUp node): the gradient is handed over as that node's space-to-depth bf16 operand
        (hn_seg_loss_bwd_s2d) instead of an fp32 dlogits tensor"""
        n, h, w, c = logits.shape
        ctx.valid = valid = None if valid is None else _task_valid_row(valid, n, logits.device)
        hw = h * w
        ctx.slot = slot if (slot is not None and h % 2 == 0 and w % 2 == 0) else None
        ctx.hw_dims = (h, w)
        k = int(top_k_ratio * hw) if use_top_k else hw
        dev = logits.device
        ws = torch.empty((lib().query("hn_seg_loss_ws_bytes", n, hw),), device=dev, dtype=torch.uint8)
        out = torch.empty((1,), device=dev, dtype=F32)
        tf = 1 if target.dtype == torch.float32 else 0
        assert target.dtype in (torch.float32, torch.int64) and target.is_contiguous()
        lib().call(_masked("hn_seg_loss_fwd", valid), ptr(logits), logits.stride(2), c, ptr(target), tf, ptr(class_weights), ignore_index, n, hw,
                   1 if use_top_k else 0, k, *_v(valid), ptr(ws), ptr(out))
        ctx.meta = (n, hw, c, tf, 1 if use_top_k else 0, k, ignore_index)
        ctx.save_for_backward(logits, target, class_weights, ws)
        return out.view(())

    @staticmethod
    def backward(ctx, gout):
        logits, target, cw, ws = ctx.saved_tensors
        n, hw, c, tf, topk, k, ign = ctx.meta
        valid = ctx.valid
        g = gout.contiguous().to(F32).view(1)
        if ctx.slot is not None and ctx.slot.buf is None:
            h, w = ctx.hw_dims
            dz = new_act(n, h // 2, w // 2, pad8(4 * c), logits.device)
            lib().call(_masked("hn_seg_loss_bwd_s2d", valid), ptr(logits), logits.stride(2), c, ptr(target), tf, ptr(cw), ign, n, h, w, topk, k,
                       *_v(valid), ptr(ws), ptr(g), ptr(dz), ld(dz))
            ctx.slot.buf = dz
            return None, None, None, None, None, None, None, None
        dl = torch.empty_like(logits)
        lib().call(_masked("hn_seg_loss_bwd", valid), ptr(logits), logits.stride(2), c, ptr(target), tf, ptr(cw), ign, n, hw, topk, k,
                   *_v(valid), ptr(ws), ptr(g), ptr(dl), dl.stride(2))
        return dl, None, None, None, None, None, None, None


def seg_loss_hip(seg_nchw, target, class_weights, use_top_k, top_k_ratio, ignore_index=255, slot=None, valid=None):
    """seg_nchw: the module's "seg" output (fp32, NCHW-shaped view of NHWC memory).  slot: GradSlot of the SegOutUp node that produced
    exactly this tensor (HydraNet passes it when its own cal_loss consumes its own "seg" output).  valid: the seg row of the task masks
    (see _task_valid_row): sum over the labelled images of their top-k sums / (N_valid k), each image's selection as without a mask."""
    logits = seg_nchw.permute(0, 2, 3, 1)
    if not logits.is_contiguous():
        logits, slot = logits.contiguous(), None
    if valid is None:
        return SegLoss.apply(logits, target.contiguous(), class_weights, use_top_k, top_k_ratio, ignore_index, slot)
    return SegLoss.apply(logits, target.contiguous(), class_weights, use_top_k, top_k_ratio, ignore_index, slot, valid)


class SegFocalLoss(torch.autograd.Function):
    """focal variant of the seg loss (head_seg/segmentation_loss.py:31-46): logits fp32 NHWC [N, H, W, C] (dense rows), target [N, H, W]
    int64 or float32 class ids; mean over all pixels"""

    @staticmethod
    def forward(ctx, logits, target, class_weights, gamma, alpha, valid=None):
        n, h, w, c = logits.shape
        ctx.valid = valid = None if valid is None else _task_valid_row(valid, n, logits.device)
        hw = h * w
        dev = logits.device
        tf = 1 if target.dtype == torch.float32 else 0
        assert target.dtype in (torch.float32, torch.int64) and target.is_contiguous()
        ws = torch.empty((lib().query("hn_seg_loss_blocks", n, hw),), device=dev, dtype=F32)
        out = torch.empty((1,), device=dev, dtype=F32)
        lib().call(_masked("hn_seg_focal_fwd", valid), ptr(logits), logits.stride(2), c, ptr(target), tf, ptr(class_weights), float(gamma),
                   float(alpha), n, hw, *_v(valid), ptr(ws), ptr(out))
        ctx.meta = (n, hw, c, tf, float(gamma), float(alpha))
        ctx.save_for_backward(logits, target, class_weights)
        return out.view(())

    @staticmethod
    def backward(ctx, gout):
        logits, target, cw = ctx.saved_tensors
        n, hw, c, tf, gamma, alpha = ctx.meta
        g = gout.contiguous().to(F32).view(1)
        dl = torch.empty_like(logits)
        lib().call(_masked("hn_seg_focal_bwd", ctx.valid), ptr(logits), logits.stride(2), c, ptr(target), tf, ptr(cw), gamma, alpha, n, hw,
                   *_v(ctx.valid), ptr(g), ptr(dl), dl.stride(2))
        return dl, None, None, None, None, None


def seg_focal_loss_hip(seg_nchw, target, class_weights, gamma=2.0, alpha=1.0, valid=None):
    """CrossEntropyLoss.forward with use_focal=True (gamma 2, alpha 1: the defaults model.py:119-124 leaves untouched).  valid: the seg
    row of the task masks: the mean over the labelled images' pixels."""
    logits = seg_nchw.permute(0, 2, 3, 1)
    if not logits.is_contiguous():
        logits = logits.contiguous()
    if valid is None:
        return SegFocalLoss.apply(logits, target.contiguous(), class_weights, gamma, alpha)
    return SegFocalLoss.apply(logits, target.contiguous(), class_weights, gamma, alpha, valid)


class SegLovaszLoss(torch.autograd.Function):
    """Lovasz-softmax variant of the seg loss (head_seg/loss_lovasz.py lovasz_softmax on softmax(logits), classes='present', per_image=False):
    logits fp32 NHWC [N, H, W, C] (dense rows), target [N, H, W] int64 or float32 class ids.  The per-class sorts, weights and per-pixel
    gradient live in the workspace the backward reads (hn_lovasz.hip)."""

    @staticmethod
    def forward(ctx, logits, target, ignore_index, slot=None, valid=None):
        """slot: GradSlot of the producing SegOutUp node, as for SegLoss (hn_seg_lovasz_bwd_s2d hands the gradient over in its operand form)"""
        n, h, w, c = logits.shape
        ctx.valid = valid = None if valid is None else _task_valid_row(valid, n, logits.device)
        hw = h * w
        ctx.slot = slot if (slot is not None and h % 2 == 0 and w % 2 == 0) else None
        ctx.hw_dims = (h, w)
        dev = logits.device
        ws = torch.empty((lib().query("hn_seg_lovasz_ws_bytes", n, hw, c),), device=dev, dtype=torch.uint8)
        out = torch.empty((1,), device=dev, dtype=F32)
        tf = 1 if target.dtype == torch.float32 else 0
        assert target.dtype in (torch.float32, torch.int64) and target.is_contiguous()
        lib().call(_masked("hn_seg_lovasz_fwd", valid), ptr(logits), logits.stride(2), c, ptr(target), tf, ignore_index, n, hw, *_v(valid),
                   ptr(ws), ptr(out))
        ctx.meta = (n, hw, c, tf, ignore_index)
        ctx.save_for_backward(logits, target, ws)
        return out.view(())

    @staticmethod
    def backward(ctx, gout):
        logits, target, ws = ctx.saved_tensors
        n, hw, c, tf, ign = ctx.meta
        valid = ctx.valid
        g = gout.contiguous().to(F32).view(1)
        if ctx.slot is not None and ctx.slot.buf is None:
            h, w = ctx.hw_dims
            dz = new_act(n, h // 2, w // 2, pad8(4 * c), logits.device)
            lib().call(_masked("hn_seg_lovasz_bwd_s2d", valid), ptr(logits), logits.stride(2), c, ptr(target), tf, ign, n, h, w, *_v(valid),
                       ptr(ws), ptr(g), ptr(dz), ld(dz))
            ctx.slot.buf = dz
            return None, None, None, None, None
        dl = torch.empty_like(logits)
        lib().call(_masked("hn_seg_lovasz_bwd", valid), ptr(logits), logits.stride(2), c, ptr(target), tf, ign, n, hw, *_v(valid), ptr(ws),
                   ptr(g), ptr(dl), dl.stride(2))
        return dl, None, None, None, None


def seg_lovasz_loss_hip(seg_nchw, target, ignore_index=255, slot=None, valid=None):
    """model.py cal_loss with use_lovasz: lovasz_softmax(F.softmax(seg, 1), gt_seg.long(), ignore=255).  seg_nchw: the module's "seg"
    output (fp32, NCHW-shaped view of NHWC memory); slot as for seg_loss_hip.  valid: the seg row of the task masks: an unlabelled
    image's pixels are dropped like ignored pixels (class presence, ranks and the tie order come from the remaining ones)."""
    logits = seg_nchw.permute(0, 2, 3, 1)
    if not logits.is_contiguous():
        logits, slot = logits.contiguous(), None
    if valid is None:
        return SegLovaszLoss.apply(logits, target.contiguous(), ignore_index, slot)
    return SegLovaszLoss.apply(logits, target.contiguous(), ignore_index, slot, valid)


def argmax_channels(seg_nchw):
    logits = seg_nchw.permute(0, 2, 3, 1)
    if not logits.is_contiguous():
        logits = logits.contiguous()
    n, h, w, c = logits.shape
    out = torch.empty((n, h, w), device=logits.device, dtype=torch.int64)
    lib().call("hn_argmax_channels", ptr(logits), logits.stride(2), c, n * h * w, ptr(out))
    return out


# --------------------------------------------------------------------------------------------------------------
# detection loss (IoU or given anchor assignment; focal / qfl / vfl classification; smooth-L1 / giou / diou / ciou regression)
# --------------------------------------------------------------------------------------------------------------
DET_IOU_KINDS = {"giou": 1, "diou": 2, "ciou": 3}
DET_CLS_KINDS = {"focal": 0, "qfl": 1, "vfl": 2}


def _det_entry(which, reg_kind, cls_kind, given, valid, aligned=False):
    """(entry-point name, the arguments between Mx and the buffers) of the detection loss's forward (which = "fwd") or backward ("bwd")
    for reg_kind 0 (smooth-L1) | DET_IOU_KINDS, cls_kind of DET_CLS_KINDS, an assignment handed in or not, a mask row or None; aligned:
    the quality pair that reads a target after the assignment"""
    if cls_kind:       # one pair of names takes the mask and the given assignment as (nullable) arguments
        name = "hn_det_loss_aligned_" if aligned else "hn_det_loss_quality_"
        return name + which, (reg_kind, cls_kind, ptr(valid)) + ((int(given),) if which == "fwd" else ())
    name = ("hn_det_loss_iou_" if reg_kind else "hn_det_loss_") + which + ("_assigned" if given and which == "fwd" else "")
    return _masked(name, valid), ((reg_kind,) if reg_kind else ()) + tuple(_v(valid))


class DetLoss(torch.autograd.Function):
    """The detection loss of hn_det_loss.hip for every pair of terms: (classification loss, regression loss), both batch means like
    FocalLoss.forward, and with an IoU-family regression term (reg_kind != 0) the mean IoU of the positives as a third output, a
    diagnostic and not differentiable."""

    @staticmethod
    def forward(ctx, cls, reg, anchors, ann, reg_kind=0, cls_kind=0, given=None, valid=None, target=None):
        n, a, k = cls.shape
        mx = ann.shape[1]
        dev = cls.device
        ctx.valid = valid = None if valid is None else _task_valid_row(valid, n, dev)
        cls, reg, ann = cls.contiguous(), reg.contiguous(), ann.contiguous().float()
        anc = anchors.reshape(-1, 4).contiguous()
        blocks = lib().query("hn_det_loss_blocks", a)
        part = torch.empty((n, blocks, 4 if reg_kind else 3), device=dev, dtype=F32)
        npos = torch.empty((n,), device=dev, dtype=F32)
        out = torch.empty((3 if reg_kind else 2,), device=dev, dtype=F32)
        assign = torch.empty((n, a), device=dev, dtype=torch.int16) if given is None else _given_assign(given, n, a, dev)
        if target is not None:
            target = _given_target(target, given, n, a, dev)
        tgt = () if target is None else (ptr(target),)
        name, args = _det_entry("fwd", reg_kind, cls_kind, given is not None, valid, target is not None)
        lib().call(name, ptr(cls), ptr(reg), ptr(anc), ptr(ann), n, a, k, mx, *args, ptr(assign), *tgt, ptr(part), ptr(npos), ptr(out))
        ctx.kinds = (reg_kind, cls_kind)
        ctx.save_for_backward(cls, reg, anc, ann, assign, npos, target)
        # the losses leave as separate outputs (slicing a 2-vector OUTSIDE the node cost two SliceBackward nodes -- fill + copy each -- and
        # an add per step: seven 5 us launches)
        if not reg_kind:
            return out[0:1], out[1:2]
        pos_iou = out[2:3]
        ctx.mark_non_differentiable(pos_iou)
        ctx.set_materialize_grads(False)        # (no zero-filled "gradient" of the diagnostic: a fill launch per step)
        return out[0:1], out[1:2], pos_iou

    @staticmethod
    def backward(ctx, gcls, greg, _giou=None):
        cls, reg, anc, ann, assign, npos, target = ctx.saved_tensors
        n, a, k = cls.shape
        tgt = () if target is None else (ptr(target),)
        dcls, dreg = torch.empty_like(cls), torch.empty_like(reg)
        if (gcls is not None and greg is not None and gcls.dtype == F32 and greg.dtype == F32
                and greg.data_ptr() == gcls.data_ptr() + 4):       # neighbours in WeightedLossSum.backward's gradient vector: used in place
            g = gcls
        else:
            z = zeros((1,), cls.device)
            g = torch.cat([(gcls if gcls is not None else z).reshape(1).to(F32), (greg if greg is not None else z).reshape(1).to(F32)])
        name, args = _det_entry("bwd", *ctx.kinds, False, ctx.valid, target is not None)
        lib().call(name, ptr(cls), ptr(reg), ptr(anc), ptr(ann), n, a, k, ann.shape[1], *args, ptr(assign), *tgt, ptr(npos), ptr(g), ptr(dcls),
                   ptr(dreg))
        return dcls, dreg, None, None, None, None, None, None, None


def _given_assign(assign, n, a, dev):
    """an assignment handed to a detection loss: int16 [N, A] on the loss's device"""
    if assign.dtype != torch.int16 or tuple(assign.shape) != (n, a) or assign.device != dev:
        raise ValueError(f"assign must be an int16 [{n}, {a}] tensor on {dev}, got {assign.dtype} {tuple(assign.shape)} on {assign.device}")
    return assign.contiguous()


def _given_target(target, assign, n, a, dev):
    """a classification target handed to a quality loss next to its assignment: fp32 [N, A] on the loss's device"""
    if assign is None:
        raise ValueError("target belongs to a given assignment: pass assign as well (det_tal_assign returns both)")
    if target.dtype != F32 or tuple(target.shape) != (n, a) or target.device != dev:
        raise ValueError(f"target must be an fp32 [{n}, {a}] tensor on {dev}, got {target.dtype} {tuple(target.shape)} on {target.device}")
    return target.detach().contiguous()


def det_loss_hip(classification, regression, anchors, annotations, assign=None, valid=None):
    """assign: None = the reference's max-IoU assignment, computed inside the forward launch; an int16 [N, A] tensor (det_atss_assign's)
    is read instead (hn_det_loss_fwd_assigned).  valid: the det row of the task masks: an unlabelled image's anchors are all ignored
    (npos 0; -2 throughout its row of a computed assignment) and the batch means are taken over the labelled images."""
    if assign is None and valid is None:
        return DetLoss.apply(classification, regression, anchors, annotations)
    return DetLoss.apply(classification, regression, anchors, annotations, 0, 0, assign, valid)


def det_atss_assign(anchors, level_sizes, annotations, topk=9, anchors_per_location=9):
    """ATSS (adaptive training sample selection) anchor assignment on HIP kernels (hn_det_atss.hip, three launches, no host
    synchronisation, capturable).  anchors [A, 4] or [1, A, 4] fp32 (y1, x1, y2, x2); level_sizes: the sizes of the contiguous anchor
    ranges of the pyramid levels (HydraNet.anchor_level_sizes), summing to A; annotations [N, Mx, 5] (x1, y1, x2, y2, class), class -1
    marks padding.  Returns (assign int16 [N, A]: the matched annotation's index or -1, thr fp32 [N, Mx]: undefined for padding rows).

    The rule, per image:
      1. An image without valid annotations has every anchor -1 (background).
      2. Centres: acy = (y1 + y2) * 0.5f, acx = (x1 + x2) * 0.5f of an anchor; gcx = (x1 + x2) * 0.5f, gcy = (y1 + y2) * 0.5f of a box.
      3. Distance d2 = dx*dx + dy*dy with dx = acx - gcx, dy = acy - gcy; every operation is an individually rounded fp32 operation
         (no fused multiply-add), so a numpy float32 restatement reproduces it bit for bit.
      4. Levels are the contiguous anchor ranges given by level_sizes.
      5. On level l with A_l anchors the candidates of a box are the k_l = min(topk * anchors_per_location, A_l) anchors with the
         smallest (d2, anchor index): ties in d2 go to the lower index.  The anchors of one location share a centre, so topk counts
         locations, as in the ATSS authors' code.
      6. IoU is the max-IoU assignment's formula (inter / max(area_a + area_b - inter, 1e-8)) in fp32.
      7. Over all of a box's candidates (n = sum of k_l) thr = mean + std of their IoUs; std is unbiased (n - 1), taken in two passes,
         and 0 when n < 2.
      8. A candidate is positive for the box when iou >= thr and min(acx - x1, acy - y1, x2 - acx, y2 - acy) > 0.01.
      9. An anchor positive for several boxes goes to the one with the largest IoU; ties go to the lowest annotation index.
     10. Every other anchor is -1.  There is no ignore zone: -2 never appears."""
    anc = anchors.reshape(-1, 4).contiguous()
    ann = annotations.contiguous().float()
    if anc.dtype != F32 or ann.dim() != 3 or ann.shape[2] != 5:
        raise ValueError("anchors must be fp32 [A, 4] and annotations [N, Mx, 5]")
    n, mx, a, dev = ann.shape[0], ann.shape[1], anc.shape[0], anc.device
    sizes = (ctypes.c_int * len(level_sizes))(*[int(v) for v in level_sizes])
    args = (ctypes.addressof(sizes), len(level_sizes), int(topk), int(anchors_per_location))
    nbytes = lib().query("hn_det_atss_ws_bytes", n, a, mx, *args)
    if nbytes < 0:
        raise ValueError(f"det_atss_assign: level_sizes {list(level_sizes)} must be 1..8 positive sizes summing to A = {a}, topk >= 1 and "
                         f"topk * anchors_per_location <= 1024 (got {topk} * {anchors_per_location})")
    ws = torch.empty((nbytes,), device=dev, dtype=torch.uint8)
    assign = torch.empty((n, a), device=dev, dtype=torch.int16)
    thr = torch.empty((n, mx), device=dev, dtype=F32)
    lib().call("hn_det_atss_assign", ptr(anc), ptr(ann), n, a, mx, *args, ptr(ws), ptr(assign), ptr(thr))
    return assign, thr


def det_tal_assign(anchors, regression, classification, annotations, topk=13):
    """Task-aligned anchor assignment (TAL; Feng et al., TOOD, 2021) on HIP kernels (hn_det_tal.hip, three launches, no host
    synchronisation, capturable).  anchors [A, 4] or [1, A, 4] fp32 (y1, x1, y2, x2); regression [N, A, 4] fp32 (dy, dx, dh, dw);
    classification [N, A, K] fp32, post-sigmoid; annotations [N, Mx, 5] (x1, y1, x2, y2, class), class -1 marks padding.  Both
    predictions are detached and read as constants: no gradient flows through the assigner.  Returns (assign int16 [N, A]: the matched
    annotation's index or -1, target fp32 [N, A]: the aligned classification target of an assigned anchor, else 0), which
    det_iou_loss_hip(..., assign=, target=) reads.  alpha = 1 and beta = 6 are fixed.

    The rule, per image, with k = topk:
      1. An image without valid annotations has every anchor -1 and every target 0.
      2. u(a, j) is the `iou` of det_iou_loss_hip's box function for anchor a's regression against box j: the deploy decode with the
         log(1000/16) clip on dh and dw, target sides clamped to at least 1, eps 1e-7 (the same device function on the same inputs as
         the loss).
      3. s(a, j) = classification[a, class_j], unclamped.  A class id outside 0 .. K - 1 gives s = 0.
      4. t(a, j) = s * ((u*u)*(u*u)) * (u*u) in fp32.
      5. Anchor a is eligible for box j when its centre lies inside the raw annotation by more than 0.01 px (ATSS's rule 8:
         min(acx - x1, acy - y1, x2 - acx, y2 - acy) > 0.01) and t > 0.  A NaN or zero metric is never eligible; a NaN anywhere in the
         anchor's regression makes its t NaN.
      6. The candidates of box j are its k eligible anchors with the largest (t, then lower anchor index); all of them if fewer than k
         are eligible.
      7. An anchor that is a candidate of several boxes goes to the box with the largest u.  Ties go to the lowest annotation index.
      8. Every other anchor is -1.  There is no ignore zone: -2 never appears.
      9. For box j, tmax and umax are the maxima of t and u over the anchors finally assigned to j, after rule 7.  The target of an
         assigned anchor is (t / tmax) * umax, both operations individually rounded.  Every other anchor's target is 0.
    Padding rows are never read."""
    anc = anchors.detach().reshape(-1, 4).contiguous()
    reg = regression.detach().contiguous()
    cls = classification.detach().contiguous()
    ann = annotations.detach().contiguous().float()
    if anc.dtype != F32 or ann.dim() != 3 or ann.shape[2] != 5:
        raise ValueError("anchors must be fp32 [A, 4] and annotations [N, Mx, 5]")
    n, mx, a, dev = ann.shape[0], ann.shape[1], anc.shape[0], anc.device
    if reg.dtype != F32 or tuple(reg.shape) != (n, a, 4) or cls.dtype != F32 or cls.dim() != 3 or tuple(cls.shape[:2]) != (n, a):
        raise ValueError(f"regression must be fp32 [{n}, {a}, 4] and classification fp32 [{n}, {a}, K], got {reg.dtype} {tuple(reg.shape)} "
                         f"and {cls.dtype} {tuple(cls.shape)}")
    nbytes = lib().query("hn_det_tal_ws_bytes", n, a, mx, int(topk))
    if nbytes < 0:
        raise ValueError(f"det_tal_assign: needs 1 <= N <= 65535, 1 <= Mx <= 32767, A >= 1 and 1 <= topk <= 2048, got N = {n}, Mx = {mx}, "
                         f"A = {a}, topk = {topk}")
    ws = torch.empty((nbytes,), device=dev, dtype=torch.uint8)
    assign = torch.empty((n, a), device=dev, dtype=torch.int16)
    target = torch.empty((n, a), device=dev, dtype=F32)
    lib().call("hn_det_tal_assign", ptr(anc), ptr(reg), ptr(cls), ptr(ann), n, a, cls.shape[2], mx, int(topk), ptr(ws), ptr(assign), ptr(target))
    return assign, target


def det_iou_loss_hip(classification, regression, anchors, annotations, kind, assign=None, valid=None, cls_kind="focal", target=None):
    """The detection loss with its regression term replaced by an IoU-family loss; kind = "giou" | "diou" | "ciou".  Returns
    (classification loss [1], regression loss [1], pos_iou [1]).  Anchor assignment (IoU >= 0.5 positive, < 0.4 background, between
    ignored, first maximum wins, an image without boxes all background) and the focal classification loss are det_loss_hip's, bit for
    bit.  For a positive anchor (ay1, ax1, ay2, ax2) with regression (dy, dx, dh, dw) and matched annotation (x1, y1, x2, y2):

      predicted box   the deploy decode (BBoxTransform, head_detect/detection_loss.py:19-33): ha = ay2 - ay1, wa = ax2 - ax1,
                      cya = (ay1 + ay2) / 2, cxa = (ax1 + ax2) / 2; cy = dy ha + cya, cx = dx wa + cxa; h = exp(min(dh, C)) ha,
                      w = exp(min(dw, C)) wa with C = log(1000 / 16).  The clip keeps one large dh of a bf16 forward from overflowing
                      exp and making the loss non-finite; the gradient w.r.t. dh / dw is zero where it is active.
      target box      the annotation's centre (gcx, gcy) with gw = max(x2 - x1, 1), gh = max(y2 - y1, 1): the smooth-L1 targets' clamp
      iou             eps = 1e-7; iw, ih = the overlap of the two boxes along x, y; inter = max(0, iw) max(0, ih);
                      union = w h + gw gh - inter + eps; iou = inter / union
      enclosing box   the smallest box around both, sides cw, ch
      giou            ac = cw ch + eps; loss = 1 - iou + (ac - union) / ac
      diou            rho2 = (cx - gcx)^2 + (cy - gcy)^2; c2 = cw^2 + ch^2 + eps; loss = 1 - iou + rho2 / c2
      ciou            diou + alpha v; v = (4 / pi^2) (atan(gw / gh) - atan(w / h))^2; alpha = v / (1 - iou + v + eps), a constant in
                      the backward (the published form)

    Per image the regression loss is sum_pos loss / npos (0 when npos = 0) and the output the mean over the N images: the smooth-L1
    term's reduction without its x4.  pos_iou is the positives' plain iou reduced the same way (non-differentiable).

    assign: None = the assignment above; an int16 [N, A] tensor (det_atss_assign's) is read instead (hn_det_loss_iou_fwd_assigned).
    valid: the det row of the task masks, as for det_loss_hip; pos_iou is averaged over the labelled images as well.

    cls_kind: "focal" (the default) makes exactly the calls above.  "qfl" (quality focal loss, Li et al. 2020) and "vfl" (varifocal
    loss, Zhang et al. 2021) replace the classification term by one whose target is the quality of the box (hn_det_loss.hip); the
    assignment, the regression loss, pos_iou and the regression gradient stay the focal call's, bit for bit.  For a counted anchor
    (assignment not -2: ignored anchors and every anchor of an unlabelled image contribute nothing and get gradient 0) and class k:

      quality         q = the `iou` above of a positive anchor: the deploy decode with the exp clip, the target sides clamped to at least
                      1, eps = 1e-7.  q is a constant in the backward: the classification term sends no gradient to the regression.
      target          y = q when the anchor is positive and k is its annotation's class, else y = 0; a class id outside 0 .. K - 1
                      matches no k
      probability     p^ = clamp(p, 1e-4, 1 - 1e-4) as in the focal loss; the gradient w.r.t. p is 0 unless 1e-4 < p < 1 - 1e-4
      BCE(p^, y)      -(y ln p^ + (1 - y) ln(1 - p^))
      qfl (beta 2)    l = (y - p^)^2 BCE(p^, y);  dl/dp = 2 (p - y) BCE + (p - y)^2 ((1 - y) / (1 - p) - y / p)
      vfl, y > 0      l = y BCE(p^, y);  dl/dp = y ((1 - y) / (1 - p) - y / p)
      vfl, y = 0      (alpha 0.75, gamma 2; includes a positive whose q is exactly 0)  l = 0.75 p^^2 (-ln(1 - p^));
                      dl/dp = 0.75 (-2 p ln(1 - p) + p^2 / (1 - p))

    Per image the sum of l over counted anchors and classes is divided by max(npos, 1); the output is the mean over the images (over
    the labelled images under a mask, 0 without any): the focal term's reduction.  beta, alpha and gamma are fixed.

    target: None, or with cls_kind "qfl" / "vfl" and an assign an fp32 [N, A] tensor (det_tal_assign's): a positive anchor's y is
    target[n, a] instead of q, a constant in the forward and in the backward (hn_det_loss_aligned_fwd / _bwd).  The regression loss,
    pos_iou and the regression gradient do not read it."""
    if kind not in DET_IOU_KINDS:
        raise ValueError(f"kind must be one of {sorted(DET_IOU_KINDS)}, got {kind!r}")
    if cls_kind not in DET_CLS_KINDS:
        raise ValueError(f"cls_kind must be one of {sorted(DET_CLS_KINDS)}, got {cls_kind!r}")
    if target is not None:
        if cls_kind == "focal":
            raise ValueError("target needs cls_kind 'qfl' or 'vfl': the focal term's target is 0 / 1")
        return DetLoss.apply(classification, regression, anchors, annotations, DET_IOU_KINDS[kind], DET_CLS_KINDS[cls_kind], assign, valid, target)
    if cls_kind == "focal" and assign is None and valid is None:
        return DetLoss.apply(classification, regression, anchors, annotations, DET_IOU_KINDS[kind])
    return DetLoss.apply(classification, regression, anchors, annotations, DET_IOU_KINDS[kind], DET_CLS_KINDS[cls_kind], assign, valid)



# --------------------------------------------------------------------------------------------------------------
# Lane losses on the device (head_lane/lanedetect_loss.py:18-78): one workgroup does the OHEM classification loss (log-softmax, counts,
# radix select of the k-th smallest background log-prob instead of torch.sort/topk, both sums); the location loss is a row kernel + a
# one-block finalize.  ~5 launches instead of ~60 tiny torch ops, and no memcpy nodes in the captured step.
# --------------------------------------------------------------------------------------------------------------
class LaneClsLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, cls_targets, cls_preds, negative_ratio, alpha, valid=None, rows=None):
        tgt = cls_targets.reshape(-1, 2).float().contiguous()
        z = cls_preds.reshape(-1, 2).float().contiguous()
        m = z.shape[0]
        dev = z.device
        ctx.valid = ctx.rows = None
        if valid is not None:
            rows = int(rows)
            if rows < 1 or m % rows:
                raise ValueError(f"rows_per_image = {rows} does not divide the {m} lane rows")
            ctx.valid, ctx.rows = _task_valid_row(valid, m // rows, dev), rows
        lsm = torch.empty((m, 2), device=dev, dtype=F32)
        pmask = torch.empty((m,), device=dev, dtype=torch.uint8)
        out = torch.empty((2,), device=dev, dtype=F32)
        aux = torch.empty((4,), device=dev, dtype=F32)
        if valid is None:
            lib().call("hn_lane_cls_loss_fwd", ptr(z), ptr(tgt), m, float(negative_ratio), float(alpha), ptr(lsm), ptr(pmask), ptr(out), ptr(aux))
        else:
            lib().call("hn_lane_cls_loss_fwd_masked", ptr(z), ptr(tgt), m, rows, ptr(valid), float(negative_ratio), float(alpha), ptr(lsm),
                       ptr(pmask), ptr(out), ptr(aux))
        ctx.alpha, ctx.shape = float(alpha), cls_preds.shape
        ctx.save_for_backward(lsm, pmask, aux)
        ctx.mark_non_differentiable(pmask, aux)
        ctx.set_materialize_grads(False)        # (no zero-filled "gradients" of the byte mask and the aux vector: two fill launches per step)
        return out[0], out[1], pmask, aux

    @staticmethod
    def backward(ctx, gpos, gneg, _gm, _ga):
        lsm, pmask, aux = ctx.saved_tensors
        m = lsm.shape[0]
        dz = torch.empty((m, 2), device=lsm.device, dtype=F32)
        gp = gpos.reshape(1).to(F32) if gpos is not None else zeros((1,), lsm.device)
        gn = gneg.reshape(1).to(F32) if gneg is not None else zeros((1,), lsm.device)
        if ctx.valid is None:
            lib().call("hn_lane_cls_loss_bwd", ptr(lsm), ptr(pmask), ptr(aux), ptr(gp), ptr(gn), ctx.alpha, m, ptr(dz))
        else:
            lib().call("hn_lane_cls_loss_bwd_masked", ptr(lsm), ptr(pmask), ptr(aux), ptr(gp), ptr(gn), ctx.alpha, m, ctx.rows, ptr(ctx.valid),
                       ptr(dz))
        return None, dz.view(ctx.shape), None, None, None, None


class LaneLocLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pmask, aux, loc_targets, loc_preds, wcol, alpha):
        L = loc_preds.shape[-1]
        if wcol + 1 >= L:
            raise IndexError(f"index {wcol + 1} is out of bounds for dimension 1 with size {L}")   # the reference's own failure mode
        p = loc_preds.reshape(-1, L).float().contiguous()
        t = loc_targets.reshape(-1, L).float().contiguous()
        m = p.shape[0]
        dev = p.device
        rowloss = torch.empty((m,), device=dev, dtype=F32)
        rownorm = torch.empty((m,), device=dev, dtype=F32)
        out = torch.empty((1,), device=dev, dtype=F32)
        lib().call("hn_lane_loc_loss_fwd", ptr(p), ptr(t), ptr(pmask), ptr(aux), m, L, int(wcol), float(alpha), ptr(rowloss), ptr(rownorm),
                   ptr(out))
        ctx.meta = (int(wcol), float(alpha), loc_preds.shape)
        ctx.save_for_backward(p, t, pmask, rownorm, aux)
        return out[0]

    @staticmethod
    def backward(ctx, gout):
        p, t, pmask, rownorm, aux = ctx.saved_tensors
        wcol, alpha, shape = ctx.meta
        m, L = p.shape
        dp = torch.empty((m, L), device=p.device, dtype=F32)
        g = gout.reshape(1).to(F32)
        lib().call("hn_lane_loc_loss_bwd", ptr(p), ptr(t), ptr(pmask), ptr(rownorm), ptr(aux), ptr(g), m, L, wcol, alpha, ptr(dp))
        return None, None, None, dp.view(shape), None, None


def _lane_rows(valid, rows_per_image, m):
    """rows per image of a masked lane loss: as given, else the row count over the mask's images"""
    if rows_per_image is not None:
        return int(rows_per_image)
    n = valid.shape[0] if isinstance(valid, torch.Tensor) and valid.dim() == 1 and valid.shape[0] > 0 else 1
    return m // n if m % n == 0 else 0


def lane_cls_loss_hip(cls_targets, cls_preds, negative_ratio=15, alpha=10.0, valid=None, rows_per_image=None):
    """cal_loss_cls (lanedetect_loss.py:18-54): returns (pos, neg, pmask, positive_num) like the reference; pmask / positive_num are
    device-side handles (byte mask, aux vector) consumed by lane_loc_loss_hip.  valid: the lane row of the task masks, with
    rows_per_image anchors rows per image (default: the row count over the mask's length): the rows of an unlabelled image are neither
    positive nor negative -- out of #pos, #neg, the rank neg_num, the select and both sums."""
    if valid is None:
        return LaneClsLoss.apply(cls_targets, cls_preds, negative_ratio, alpha)
    return LaneClsLoss.apply(cls_targets, cls_preds, negative_ratio, alpha, valid, _lane_rows(valid, rows_per_image, cls_preds.numel() // 2))


def lane_loc_loss_hip(pmask, positive_num, loc_targets, loc_preds, alpha=10.0, points_per_line=160, valid=None, rows_per_image=None):
    """cal_loss_regress (lanedetect_loss.py:57-78) incl. its hard-coded points_per_line = 160 default (x10 weights on columns 160/161).
    valid / rows_per_image: as handed to lane_cls_loss_hip; the masked pmask / positive_num already carry the mask (an unlabelled
    image has no positive row, and only positive rows enter the loss and the gradient), so they are checked and the launches are the same."""
    if valid is not None:
        m = loc_preds.numel() // loc_preds.shape[-1]
        rows = _lane_rows(valid, rows_per_image, m)
        if rows < 1 or m % rows:
            raise ValueError(f"rows_per_image = {rows} does not divide the {m} lane rows")
        _task_valid_row(valid, m // rows, loc_preds.device)
    return LaneLocLoss.apply(pmask, positive_num, loc_targets, loc_preds, points_per_line, alpha)


class LaneLIoULoss(torch.autograd.Function):
    """The line-IoU location loss of hn_lane_liou.hip: (loss, mean line IoU of the positive rows), the second a diagnostic and not
    differentiable.  Two launches forward, one backward, as LaneLocLoss."""

    @staticmethod
    def forward(ctx, pmask, aux, loc_targets, loc_preds, ppl, e, alpha):
        L = loc_preds.shape[-1]
        p = loc_preds.reshape(-1, L).float().contiguous()
        t = loc_targets.reshape(-1, L).float().contiguous()
        m = p.shape[0]
        dev = p.device
        rows = torch.empty((4, m), device=dev, dtype=F32)            # I, U, normaliser, loss of every row
        out = torch.empty((2,), device=dev, dtype=F32)
        lib().call("hn_lane_liou_loss_fwd", ptr(p), ptr(t), ptr(pmask), ptr(aux), m, L, int(ppl), float(e), float(alpha), ptr(rows[0]),
                   ptr(rows[1]), ptr(rows[2]), ptr(rows[3]), ptr(out))
        ctx.meta = (int(ppl), float(e), float(alpha), loc_preds.shape)
        ctx.save_for_backward(p, t, pmask, rows, aux)
        pos_liou = out[1]
        ctx.mark_non_differentiable(pos_liou)
        ctx.set_materialize_grads(False)        # (no zero-filled "gradient" of the diagnostic: a fill launch per step)
        return out[0], pos_liou

    @staticmethod
    def backward(ctx, gout, _gliou=None):
        if gout is None:
            return None, None, None, None, None, None, None
        p, t, pmask, rows, aux = ctx.saved_tensors
        ppl, e, alpha, shape = ctx.meta
        m, L = p.shape
        dp = torch.empty((m, L), device=p.device, dtype=F32)
        g = gout.reshape(1).to(F32)
        lib().call("hn_lane_liou_loss_bwd", ptr(p), ptr(t), ptr(pmask), ptr(rows[1]), ptr(rows[2]), ptr(aux), ptr(g), m, L, ppl, e, alpha, ptr(dp))
        return None, None, None, dp.view(shape), None, None, None


def lane_liou_half_width(half_width):
    """the half width of a line-IoU loss as a float; ValueError unless it is a finite number > 0"""
    if isinstance(half_width, bool) or not isinstance(half_width, (int, float)) or not (0.0 < float(half_width) < float("inf")):
        raise ValueError(f"the line-IoU half width must be a finite number > 0, got {half_width!r}")
    return float(half_width)


def lane_liou_loss_hip(pmask, positive_num, loc_targets, loc_preds, half_width, alpha=10.0, points_per_line=None, valid=None, rows_per_image=None):
    """Line-IoU location loss (CLRNet, section 3.4; hn_lane_liou.hip) in place of lane_loc_loss_hip: every positive row's valid
    x-offsets are regressed as ONE thick line, 1 - sum(2e - |p - t|) / sum(2e + |p - t|) with e = half_width in the units of loc_targets,
    and its two lengths keep the smooth-L1 term (x alpha over the row's valid-column count).  -> (loss, pos_liou): pos_liou, the mean
    line IoU of the positive rows with a valid x-offset, is a detached device scalar.  points_per_line: P of the [.., 2 P + 2] rows
    (default: from the row length).  valid / rows_per_image: as for lane_loc_loss_hip (pmask / positive_num carry the mask)."""
    e = lane_liou_half_width(half_width)
    L = loc_preds.shape[-1]
    ppl = (L - 2) // 2 if points_per_line is None else int(points_per_line)
    if ppl < 1 or L != 2 * ppl + 2:
        raise ValueError(f"line-IoU rows have 2 * points_per_line + 2 columns: got {L} columns for points_per_line = {ppl}")
    if tuple(loc_targets.shape) != tuple(loc_preds.shape):
        raise ValueError(f"loc_targets {tuple(loc_targets.shape)} and loc_preds {tuple(loc_preds.shape)} differ in shape")
    if valid is not None:
        m = loc_preds.numel() // L
        rows = _lane_rows(valid, rows_per_image, m)
        if rows < 1 or m % rows:
            raise ValueError(f"rows_per_image = {rows} does not divide the {m} lane rows")
        _task_valid_row(valid, m // rows, loc_preds.device)
    return LaneLIoULoss.apply(pmask, positive_num, loc_targets, loc_preds, ppl, e, alpha)


# --------------------------------------------------------------------------------------------------------------
# HydraTrainer.cal_total_loss (model/train.py:192-203) as one launch forward and one backward instead of ~22 scalar torch kernels.
# --------------------------------------------------------------------------------------------------------------
class WeightedLossSum(torch.autograd.Function):
    """total = sum_g (sum_{i in g} x_i * w_i) * gw_g; meta = (w tuple, gw tuple, group-id tuple), xs = fp32 scalar device tensors"""

    @staticmethod
    def forward(ctx, meta, *xs):
        w, gw, grp = meta
        n = len(xs)
        ctx.shapes = [x.shape for x in xs]
        xs = [x.reshape(1) for x in xs]
        assert all(x.dtype == F32 and x.is_cuda for x in xs)
        out = torch.empty((1,), device=xs[0].device, dtype=F32)
        ctx.host = (_ptr_array(xs), (ctypes.c_float * n)(*w), (ctypes.c_float * len(gw))(*gw), (ctypes.c_int * n)(*grp), n)
        pa, wa, ga, ia, _ = ctx.host
        lib().call("hn_weighted_sum", ctypes.addressof(pa), ctypes.addressof(wa), ctypes.addressof(ga), ctypes.addressof(ia), n, None, ptr(out), None)
        ctx.keep = xs                                     # the pointer table refers to these
        return out.view(())

    @staticmethod
    def backward(ctx, gout):
        pa, wa, ga, ia, n = ctx.host
        grads = torch.empty((n,), device=gout.device, dtype=F32)
        g = gout.reshape(1)
        if g.dtype != F32:
            g = g.float()
        lib().call("hn_weighted_sum", ctypes.addressof(pa), ctypes.addressof(wa), ctypes.addressof(ga), ctypes.addressof(ia), n, ptr(g), None, ptr(grads))
        return (None, *[grads[i:i + 1].view(shape) for i, shape in enumerate(ctx.shapes)])


def weighted_loss_sum(groups):
    """groups = [(group weight, [(loss tensor, weight), ...]), ...] -> the reference's total loss, same association order"""
    xs, w, gw, grp = [], [], [], []
    for gi, (gweight, terms) in enumerate(groups):
        gw.append(float(gweight))
        for x, wi in terms:
            xs.append(x)
            w.append(float(wi))
            grp.append(gi)
    return WeightedLossSum.apply((tuple(w), tuple(gw), tuple(grp)), *xs)


# --------------------------------------------------------------------------------------------------------------
# train.loss_balance: uncertainty: the same sum under one learned log-variance per term, hn_balanced_sum.
# --------------------------------------------------------------------------------------------------------------
BALANCE_MAX_TERMS = 8                                          # HN_MAX_LOSS_TERMS


def loss_balance_clamp(clamp):
    """the clamp S of the log-variances as a float; ValueError unless it is a finite number in (0, 80] (expf(80) is finite in fp32)"""
    if isinstance(clamp, bool) or not isinstance(clamp, (int, float)) or not (0.0 < float(clamp) <= 80.0):
        raise ValueError(f"the log-variance clamp must be a number in (0, 80], got {clamp!r}")
    return float(clamp)


class BalancedLossSum(torch.autograd.Function):
    """total = [sum_g (sum_{i in g} (x_i * w_i) * exp(-s_i)) * gw_g] + sum_i s_i over the active terms (x_i != 0), s clamped to +-clamp;
    meta = (w, gw, group ids, slots, clamp, log_vars, grad_out, record): log_vars fp32 [n_slots] on the device, grad_out fp32
    [2 * n_slots] (backward writes d total / d s and the slots' activity there: a caller-owned static tensor, not a leaf's .grad),
    record fp32 [16] (forward writes exp(-s) and the activity per term)."""

    @staticmethod
    def forward(ctx, meta, *xs):
        w, gw, grp, slots, clamp, s, ds, record = meta
        n, ns = len(xs), s.numel()
        ctx.shapes = [x.shape for x in xs]
        xs = [x.reshape(1) for x in xs]
        assert all(x.dtype == F32 and x.is_cuda for x in xs)
        for t, k in ((s, ns), (ds, 2 * ns), (record, 2 * BALANCE_MAX_TERMS)):
            assert t.dtype == F32 and t.is_cuda and t.is_contiguous() and t.numel() == k and not t.requires_grad
        out = torch.empty((1,), device=xs[0].device, dtype=F32)
        ctx.host = (_ptr_array(xs), (ctypes.c_float * n)(*w), (ctypes.c_float * len(gw))(*gw), (ctypes.c_int * n)(*grp),
                    (ctypes.c_int * n)(*slots), n, ns, clamp)
        pa, wa, ga, ia, sa, _, _, _ = ctx.host
        lib().call("hn_balanced_sum", ctypes.addressof(pa), ctypes.addressof(wa), ctypes.addressof(ga), ctypes.addressof(ia),
                   ctypes.addressof(sa), n, ns, ptr(s), clamp, None, ptr(out), ptr(record), None, None)
        ctx.keep = (xs, s, ds, record)                    # the pointer table refers to these
        return out.view(())

    @staticmethod
    def backward(ctx, gout):
        pa, wa, ga, ia, sa, n, ns, clamp = ctx.host
        _, s, ds, record = ctx.keep
        grads = torch.empty((n,), device=gout.device, dtype=F32)
        g = gout.reshape(1)
        if g.dtype != F32:
            g = g.float()
        lib().call("hn_balanced_sum", ctypes.addressof(pa), ctypes.addressof(wa), ctypes.addressof(ga), ctypes.addressof(ia),
                   ctypes.addressof(sa), n, ns, ptr(s), clamp, ptr(g), None, ptr(record), ptr(grads), ptr(ds))
        return (None, *[grads[i:i + 1].view(shape) for i, shape in enumerate(ctx.shapes)])


def balanced_loss_sum(groups, log_vars, grad_out, clamp, slots=None, record=None):
    """groups = [(group weight, [(loss tensor, weight), ...]), ...] as for weighted_loss_sum -> the total under learned uncertainty
    weights.  log_vars: fp32 device tensor of the log-variances; slots: the entry of it each term owns, in term order, strictly
    increasing (default 0, 1, ...); grad_out: fp32 [2 * len(log_vars)], written by backward (d total / d log_vars, then 1.0 / 0.0 per
    slot = its term was active); record (default: a fresh tensor): fp32 [16], written by forward."""
    xs, w, gw, grp = [], [], [], []
    for gi, (gweight, terms) in enumerate(groups):
        gw.append(float(gweight))
        for x, wi in terms:
            xs.append(x)
            w.append(float(wi))
            grp.append(gi)
    slots = tuple(range(len(xs))) if slots is None else tuple(int(k) for k in slots)
    ns = log_vars.numel()
    if not xs or len(xs) > BALANCE_MAX_TERMS or ns > BALANCE_MAX_TERMS or len(slots) != len(xs):
        raise ValueError(f"balanced_loss_sum takes 1 to {BALANCE_MAX_TERMS} terms and one slot per term: got {len(xs)} terms, {len(slots)} slots, "
                         f"{ns} log-variances")
    if any(not 0 <= k < ns for k in slots) or any(b <= a for a, b in zip(slots, slots[1:])):
        raise ValueError(f"the slots {slots} are not strictly increasing indices into {ns} log-variances")
    if record is None:
        record = torch.zeros((2 * BALANCE_MAX_TERMS,), device=log_vars.device, dtype=F32)
    return BalancedLossSum.apply((tuple(w), tuple(gw), tuple(grp), slots, loss_balance_clamp(clamp), log_vars, grad_out, record), *xs)


__all__ = [n for n in dir() if not n.startswith("__")]      # everything, incl. single-underscore helpers: the package is one namespace
