"""TEST REFERENCE (not part of the product package): the losses under per-image task masks (gt_dict["task_valid"]).

The rule has no mathematics of its own: a task's masked losses are the UNMASKED losses of the sub-batch of its labelled images, taken in
batch order; without a labelled image every loss is 0; the gradient of an unlabelled image's predictions is 0.  So every function here
compacts its inputs with the mask, calls the existing float64 / integer reference (tests/loss_ref.py, det_iou_ref.py through
det_atss_ref.losses_given_assign, lovasz_ref.py) on what is left, and scatters the gradients back into zeros.  tests/
test_partial_labels_cpu.py checks that an all-ones mask gives the unmasked reference itself."""
import numpy as np
import torch

from tests import det_atss_ref, loss_ref as R, lovasz_ref

F64 = np.float64


def labelled(valid):
    """mask [N] -> indices of the labelled images, in batch order"""
    return np.flatnonzero(np.asarray(valid).reshape(-1) != 0)


def scatter(shape, idx, values):
    out = np.zeros(shape, F64)
    if len(idx):
        out[idx] = values
    return out


# ------------------------------------------------------------------------------------------------------------------------------------
# segmentation
# ------------------------------------------------------------------------------------------------------------------------------------
def seg_ce_mean(logits, target, cw, use_topk, k, valid, ignore_index=255, keys=None):
    """loss_ref.seg_ce_mean on the labelled images.  logits [N, HW, C], target [N, HW] -> (scalar, gradient [N, HW, C])"""
    idx = labelled(valid)
    if not len(idx):
        return 0.0, np.zeros(np.asarray(logits).shape, F64)
    val, grad = R.seg_ce_mean(np.asarray(logits)[idx], np.asarray(target)[idx], cw, use_topk, k, ignore_index,
                              None if keys is None else np.asarray(keys)[idx])
    return val, scatter(np.asarray(logits).shape, idx, grad)


def seg_focal(logits, target, cw, gamma, alpha, valid):
    """loss_ref.seg_focal on the labelled images' pixels.  logits [N, HW, C], target [N, HW] -> (scalar, gradient [N, HW, C])"""
    logits, target = np.asarray(logits), np.asarray(target)
    idx = labelled(valid)
    if not len(idx):
        return 0.0, np.zeros(logits.shape, F64)
    C = logits.shape[-1]
    val, grad = R.seg_focal(logits[idx].reshape(-1, C), target[idx].reshape(-1), cw, gamma, alpha)
    return val, scatter(logits.shape, idx, grad.reshape(len(idx), -1, C))


def seg_lovasz(logits_nchw, target, valid, ignore_index=255):
    """lovasz_ref.lovasz_softmax_ref on the labelled images (pixels stay in (n, h, w) order, so the stable tie order is the sub-batch's).
    logits [N, C, H, W] / target [N, H, W] torch tensors -> (scalar, gradient [N, C, H, W] float64 numpy)"""
    idx = labelled(valid)
    shape = tuple(logits_nchw.shape)
    if not len(idx):
        return 0.0, np.zeros(shape, F64)
    sel = torch.as_tensor(idx)
    x = logits_nchw.detach().cpu().double()[sel].requires_grad_(True)
    val = lovasz_ref.lovasz_softmax_ref(x, target.detach().cpu()[sel], ignore_index)
    (g,) = torch.autograd.grad(val, x, allow_unused=True)
    g = torch.zeros_like(x) if g is None else g
    return float(val.detach()), scatter(shape, idx, g.numpy())


# ------------------------------------------------------------------------------------------------------------------------------------
# detection
# ------------------------------------------------------------------------------------------------------------------------------------
def max_iou_assign(anchors, ann):
    """the max-IoU assignment of loss_ref.det_smooth_l1 (index | -1 background | -2 ignored) for ann [N, Mx, 5] -> int64 [N, A]"""
    anc = np.asarray(anchors, F64).reshape(-1, 4)
    ann = np.asarray(ann, F64)
    N, A = ann.shape[0], anc.shape[0]
    return R.det_smooth_l1(np.full((N, A, 1), 0.5), np.zeros((N, A, 4)), anc, ann)["assign"]


def det(cls, reg, anchors, ann, valid, kind="smooth_l1", assign=None, gcls=1.0, greg=1.0):
    """det_atss_ref.losses_given_assign (smooth_l1 | giou | diou | ciou) on the labelled images, under the max-IoU assignment of
    loss_ref.det_smooth_l1 (assign None) or the given one.  cls [N, A, K], reg [N, A, 4], anchors [A, 4], ann [N, Mx, 5] ->
    dict(cls, reg, pos_iou, npos [N], assign [N, A] with -2 rows for unlabelled images (None when it was given), dcls, dreg): the
    gradients of gcls * cls + greg * reg"""
    cls, reg, ann = np.asarray(cls, F64), np.asarray(reg, F64), np.asarray(ann, F64)
    anc = np.asarray(anchors, F64).reshape(-1, 4)
    N, A, _ = cls.shape
    idx = labelled(valid)
    out = dict(cls=0.0, reg=0.0, pos_iou=0.0, npos=[0] * N, assign=None if assign is not None else np.full((N, A), -2, np.int64),
               dcls=np.zeros(cls.shape, F64), dreg=np.zeros(reg.shape, F64), margin=float("inf"))
    if not len(idx):
        return out
    sub_assign = max_iou_assign(anc, ann[idx]) if assign is None else np.asarray(assign)[idx].astype(np.int64)
    c = torch.from_numpy(cls[idx]).requires_grad_(True)
    r = torch.from_numpy(reg[idx]).requires_grad_(True)
    o = det_atss_ref.losses_given_assign(c, r, torch.from_numpy(anc), torch.from_numpy(ann[idx]), sub_assign, kind)
    dc, dr = torch.autograd.grad(gcls * o["cls"] + greg * o["reg"], (c, r), allow_unused=True)
    out.update(cls=float(o["cls"].detach()), reg=float(o["reg"].detach()), pos_iou=float(o["pos_iou"]), margin=o["margin"])
    for j, n in enumerate(idx):
        out["npos"][n] = o["npos"][j]
    if assign is None:
        out["assign"][idx] = sub_assign
    out["dcls"] = scatter(cls.shape, idx, dc.numpy() if dc is not None else 0.0)
    out["dreg"] = scatter(reg.shape, idx, dr.numpy() if dr is not None else 0.0)
    return out


# ------------------------------------------------------------------------------------------------------------------------------------
# lane
# ------------------------------------------------------------------------------------------------------------------------------------
def lane_rows(valid, rows):
    """indices of the lane rows of the labelled images (rows per image), in order"""
    idx = labelled(valid)
    return (idx[:, None] * rows + np.arange(rows)[None, :]).reshape(-1)


def lane_cls(logits, target, rows, valid, neg_ratio=15.0, alpha=10.0, gpos=1.0, gneg=1.0):
    """loss_ref.lane_cls on the rows of the labelled images.  logits / target [M, 2], M = N * rows ->
    dict(pos, neg, thr, posn, npos, nneg, k, pmask bool [M], dlogits [M, 2], rows: the labelled rows' indices)"""
    z, t = np.asarray(logits), np.asarray(target)
    M = z.shape[0]
    ri = lane_rows(valid, rows)
    out = dict(pos=0.0, neg=0.0, thr=np.inf, posn=1, npos=0, nneg=0, k=1, pmask=np.zeros(M, bool), dlogits=np.zeros((M, 2), F64), rows=ri)
    if not len(ri):
        return out
    ref = R.lane_cls(z[ri], t[ri], neg_ratio, alpha, gpos, gneg)
    out.update({key: ref[key] for key in ("pos", "neg", "thr", "posn", "npos", "nneg", "k")})
    out["pmask"][ri] = ref["pmask"]
    out["dlogits"][ri] = ref["dlogits"]
    return out


def lane_select(bg_f32, rows, valid, pmask, k):
    """loss_ref.lane_select (the integer selection of the OHEM threshold) on the labelled rows of the fp32 log-probs read back"""
    ri = lane_rows(valid, rows)
    if not len(ri):
        return np.float32(np.inf)
    return R.lane_select(np.asarray(bg_f32)[ri], np.asarray(pmask, bool)[ri], k)


def lane_loc(pred, target, rows, valid, pmask, posn, wcol, alpha=10.0, gout=1.0):
    """loss_ref.lane_loc on the rows of the labelled images with the masked classification loss's pmask / posn -> (loss, dpred [M, L])"""
    p, t = np.asarray(pred), np.asarray(target)
    ri = lane_rows(valid, rows)
    if not len(ri):
        return 0.0, np.zeros(p.shape, F64)
    val, grad, _ = R.lane_loc(p[ri], t[ri], np.asarray(pmask, bool)[ri], posn, wcol, alpha, gout)
    return val, scatter(p.shape, ri, grad)
