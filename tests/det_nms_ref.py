"""numpy restatement of the detection post-process with its suppression options (hn_det_postprocess_ex): select, stable
order, class offset, then hard / DIoU greedy NMS or Soft-NMS (linear, gaussian), max_det, class-agnostic.

Everything that decides anything is float32 arithmetic, one numpy elementwise operation per rounding, in the kernels' operation order; the
gaussian weight is the float32 rounding of a float64 exp.  One vectorised pass over the candidates per selection step, no per-pair loops.
The only non-numpy call is torch's float32 exp in the box decode (the pinned oracle decodes with it; with regression 0 it is exact)."""
import numpy as np
import torch

KINDS = ("hard", "diou", "soft_linear", "soft_gaussian")
F = np.float32


def _iou(a, b):
    """a [4], b [M, 4] float32 (x1, y1, x2, y2) -> IoU [M] = inter / ((area_a + area_b) - inter); 0 / 0 is NaN"""
    area_a = (a[2] - a[0]) * (a[3] - a[1])
    area_b = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    iw = np.minimum(a[2], b[:, 2]) - np.maximum(a[0], b[:, 0])
    ih = np.minimum(a[3], b[:, 3]) - np.maximum(a[1], b[:, 1])
    iw = np.where(iw > 0, iw, F(0))
    ih = np.where(ih > 0, ih, F(0))
    inter = iw * ih
    with np.errstate(invalid="ignore", divide="ignore"):
        return inter / ((area_a + area_b) - inter)


def _diou(a, b):
    """IoU - rho^2 / c^2 (the penalty is 0 when c^2 is not > 0)"""
    iou = _iou(a, b)
    dx = (b[:, 0] + b[:, 2]) / F(2) - (a[0] + a[2]) / F(2)
    dy = (b[:, 1] + b[:, 3]) / F(2) - (a[1] + a[3]) / F(2)
    rho2 = dx * dx + dy * dy
    ex = np.maximum(a[2], b[:, 2]) - np.minimum(a[0], b[:, 0])
    ey = np.maximum(a[3], b[:, 3]) - np.minimum(a[1], b[:, 1])
    c2 = ex * ex + ey * ey
    with np.errstate(invalid="ignore", divide="ignore"):
        pen = np.where(c2 > 0, rho2 / c2, F(0)).astype(F)
    return iou - pen


def select(anchors, regression, classification, img_hw, threshold):
    """one image: anchors [A, 4] (y1, x1, y2, x2), regression [A, 4], classification [A, K] -> (anchor ids, classes, boxes, scores) of the
    anchors over the threshold in the stable order (score descending, anchor ascending), and the largest box coordinate among them"""
    an, r, c = (np.ascontiguousarray(v, dtype=F) for v in (anchors, regression, classification))
    score = c.max(axis=1)
    cls = c.argmax(axis=1)                                             # first maximum
    idx = np.nonzero(score > F(threshold))[0]
    an, r = an[idx], r[idx]
    ex = lambda v: torch.from_numpy(np.ascontiguousarray(v)).exp().numpy()
    yca, xca = (an[:, 0] + an[:, 2]) / F(2), (an[:, 1] + an[:, 3]) / F(2)
    ha, wa = an[:, 2] - an[:, 0], an[:, 3] - an[:, 1]
    w, h = ex(r[:, 3]) * wa, ex(r[:, 2]) * ha
    yc, xc = r[:, 0] * ha + yca, r[:, 1] * wa + xca
    x1, y1, x2, y2 = xc - w / F(2), yc - h / F(2), xc + w / F(2), yc + h / F(2)
    x1 = np.where(x1 < 0, F(0), x1)
    y1 = np.where(y1 < 0, F(0), y1)
    x2 = np.where(x2 > F(img_hw[1] - 1), F(img_hw[1] - 1), x2)
    y2 = np.where(y2 > F(img_hw[0] - 1), F(img_hw[0] - 1), y2)
    boxes = np.stack([x1, y1, x2, y2], axis=1).astype(F)
    order = np.argsort(-score[idx], kind="stable")                     # idx is ascending: ties keep the anchor order
    idx = idx[order]
    boxes = boxes[order]
    maxc = boxes.max() if len(idx) else F(0)
    return idx, cls[idx], boxes, score[idx], F(maxc)


def nms_image(anchors, regression, classification, img_hw, threshold, iou_threshold, kind="hard", sigma=0.5, score_floor=None, max_det=0,
              class_agnostic=False):
    """-> (anchor indices, class ids, boxes [k, 4] float32, scores [k] float32) in output order"""
    assert kind in KINDS
    idx, cls, boxes, s, maxc = select(anchors, regression, classification, img_hw, threshold)
    n = len(idx)
    thr = F(iou_threshold)
    if class_agnostic:
        b = boxes
    else:
        b = (boxes + (cls.astype(F) * (maxc + F(1)))[:, None]).astype(F)
    out, out_s = [], []
    if kind in ("hard", "diou"):
        crit = _iou if kind == "hard" else _diou
        dead = np.zeros(n, bool)
        for i in range(n):
            if dead[i]:
                continue
            if max_det and len(out) >= max_det:
                break
            out.append(i)
            out_s.append(s[i])
            with np.errstate(invalid="ignore"):
                dead[i + 1:] |= crit(b[i], b[i + 1:]) > thr              # a NaN criterion suppresses nothing
    else:
        floor = F(threshold if score_floor is None else score_floor)
        sig = np.float64(F(sigma))                                       # the C ABI carries sigma as a float
        t = s.astype(F).copy()
        alive = np.ones(n, bool)
        while alive.any():
            m = int(np.argmax(np.where(alive, t, -np.inf)))              # largest working score, ties to the smaller sorted index
            out.append(m)
            out_s.append(t[m])
            alive[m] = False
            if max_det and len(out) >= max_det:
                break
            j = np.nonzero(alive)[0]
            iou = _iou(b[m], b[j])
            with np.errstate(invalid="ignore"):
                if kind == "soft_linear":
                    w = np.where(iou > thr, F(1) - iou, F(1)).astype(F)
                else:
                    w = np.exp(-(iou.astype(np.float64) ** 2) / sig).astype(F)
                    w = np.where(np.isnan(iou), F(1), w).astype(F)
            t[j] = t[j] * w
            alive[j] = t[j] > floor
    o = np.asarray(out, dtype=np.int64)
    return idx[o], cls[o].astype(np.int64), boxes[o], np.asarray(out_s, dtype=F)


def nms_batch(anchors, regression, classification, img_hw, threshold, iou_threshold, **opts):
    """anchors [A, 4] or [1 | N, A, 4], regression [N, A, 4], classification [N, A, K] -> one nms_image tuple per image"""
    anchors, regression, classification = (np.asarray(v, dtype=F) for v in (anchors, regression, classification))
    an = anchors[0] if anchors.ndim == 3 else anchors
    return [nms_image(an, regression[i], classification[i], img_hw, threshold, iou_threshold, **opts) for i in range(len(regression))]


def count_over(classification, threshold):
    """per image, the number of anchors over the score threshold (the device pipeline's `total`)"""
    c = np.asarray(classification, dtype=F)
    return (c.max(axis=2) > F(threshold)).sum(axis=1)


# ---- the inputs the tests share: clusters of overlapping integer boxes, regression 0 (decode and clip are then exact) ------------------
def recipe(seed=7, clusters=20, per=13, frame=128, classes=3, keep=None, threshold=0.05):
    """-> (anchors [A, 4] (y1, x1, y2, x2), regression [A, 4] = 0, classification [A, classes]) of one image: cluster centres uniform
    integers in [20, frame - 20), half sizes in [10, 30), every coordinate jittered by an integer in [-12, 12] and clipped to the frame, one
    class per cluster, scores k / 4096 (equal scores occur).  keep: only the first `keep` anchors over the threshold keep their score."""
    g = np.random.default_rng(seed)
    cx, cy = g.integers(20, frame - 20, clusters), g.integers(20, frame - 20, clusters)
    hx, hy = g.integers(10, 30, clusters), g.integers(10, 30, clusters)
    kc = g.integers(0, classes, clusters)
    a = clusters * per
    jit = g.integers(-12, 13, (a, 4))
    rep = lambda v: np.repeat(v, per)
    x1, y1 = rep(cx - hx) + jit[:, 0], rep(cy - hy) + jit[:, 1]
    x2, y2 = rep(cx + hx) + jit[:, 2], rep(cy + hy) + jit[:, 3]
    anchors = np.clip(np.stack([y1, x1, y2, x2], axis=1), 0, frame - 1).astype(F)
    score = (g.integers(1, 4096, a) / 4096.0).astype(F)
    if keep is not None:
        over = np.nonzero(score > F(threshold))[0]
        assert len(over) >= keep, (len(over), keep)
        score[over[keep:]] = 0
    cls = np.zeros((a, classes), F)
    cls[np.arange(a), rep(kc)] = score
    return anchors, np.zeros((a, 4), F), cls


def batch_of(images):
    """images of recipe() with one anchor set each -> (anchors [A, 4], regression [N, A, 4], classification [N, A, K]): the device pipeline
    has ONE anchor set per batch, so the images' boxes become disjoint anchor ranges and every image scores only its own"""
    k = images[0][2].shape[1]
    anchors = np.concatenate([im[0] for im in images])
    a = len(anchors)
    reg = np.zeros((len(images), a, 4), F)
    cls = np.zeros((len(images), a, k), F)
    o = 0
    for i, im in enumerate(images):
        cls[i, o:o + len(im[0])] = im[2]
        o += len(im[0])
    return anchors, reg, cls
