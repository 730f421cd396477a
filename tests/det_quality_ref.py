"""TEST REFERENCE (not part of the product package): the detection loss with a quality classification term (detection.loss_cls_type =
qfl | vfl) restated in torch, float64 by default, as a per-image loop whose gradients come from autograd.  It restates the cls_kind part
of the docstring of multitask_hydranet_amd.ops.losses.det_iou_loss_hip; the box function and the max-IoU assignment are
tests/det_iou_ref.py's.

  counted anchor (assignment not -2), class k:  y = q when the anchor is positive and k is its annotation's class, else 0, with q the
  (detached) iou of det_iou_ref.box_losses;  p^ = clamp(p, 1e-4, 1 - 1e-4);  BCE = -(y ln p^ + (1 - y) ln(1 - p^))
  qfl  l = (y - p^)^2 BCE
  vfl  l = y BCE for y > 0,  0.75 p^^2 (-ln(1 - p^)) for y = 0
  per image sum l / max(npos, 1); mean over the images, or over the labelled ones under a valid row (0 without any)."""
import torch

from tests import det_iou_ref as R

CLS_KINDS = ("qfl", "vfl")
LO, HI = 1e-4, 1.0 - 1e-4


def bce(pc, y):
    return -(y * torch.log(pc) + (1 - y) * torch.log(1 - pc))


def term(p, y, cls_kind):
    """the loss of single (probability, target) pairs, elementwise; differentiable w.r.t. p through the clamp"""
    assert cls_kind in CLS_KINDS, cls_kind
    pc = p.clamp(LO, HI)
    if cls_kind == "qfl":
        return (y - pc) ** 2 * bce(pc, y)
    return torch.where(y > 0, y * bce(pc, y), 0.75 * pc ** 2 * -torch.log(1 - pc))


def analytic_grad(p, y, cls_kind):
    """d term / dp as the op's docstring states it (what the kernel evaluates): 0 unless 1e-4 < p < 1 - 1e-4"""
    assert cls_kind in CLS_KINDS, cls_kind
    inside = (p > LO) & (p < HI)
    q = torch.where(inside, p, torch.full_like(p, 0.5))               # (a harmless stand-in where the result is masked)
    t = (1 - y) / (1 - q) - y / q
    if cls_kind == "qfl":
        g = 2 * (q - y) * bce(q, y) + (q - y) ** 2 * t
    else:
        g = torch.where(y > 0, y * t, 0.75 * (-2 * q * torch.log(1 - q) + q ** 2 / (1 - q)))
    return torch.where(inside, g, torch.zeros_like(g))


def max_iou_assign(anc, ann):
    """anc [A, 4], ann [M, 5] of one image -> [A] long: >= 0 the matched annotation, -1 background, -2 ignored (0.4 <= best IoU < 0.5).
    Positives and their annotation are det_iou_ref.assign's; the ignore zone repeats its IoU."""
    pos, arg = R.assign(anc, ann)
    out = torch.full((anc.shape[0],), -1, dtype=torch.long)
    valid = ann[:, 4] != -1
    if bool(valid.any()):
        iw = (torch.min(anc[:, None, 3], ann[None, :, 2]) - torch.max(anc[:, None, 1], ann[None, :, 0])).clamp(min=0)
        ih = (torch.min(anc[:, None, 2], ann[None, :, 3]) - torch.max(anc[:, None, 0], ann[None, :, 1])).clamp(min=0)
        ua = ((anc[:, 2] - anc[:, 0]) * (anc[:, 3] - anc[:, 1]))[:, None] + ((ann[:, 2] - ann[:, 0]) * (ann[:, 3] - ann[:, 1]))[None, :] - iw * ih
        iou = torch.where(valid[None, :], iw * ih / ua.clamp(min=1e-8), torch.full_like(ua, -1.0))
        best = iou.max(dim=1)[0]
        out[(best >= 0.4) & ~pos] = -2
    out[pos] = arg[pos]
    return out


def det_quality_loss(classification, regression, anchors, annotations, kind, cls_kind, assign=None, valid=None, dtype=torch.float64):
    """classification [N, A, K], regression [N, A, 4], anchors [1, A, 4] or [A, 4], annotations [N, M, 5]; assign: None (the max-IoU
    assignment) or [N, A] integers (>= 0 annotation index, -1 background, -2 ignored); valid: None or N flags (1 = image labelled) ->
    dict(cls [], reg [], pos_iou [], npos [N ints; 0 for an unlabelled image], q [N tensors: the positives' quality], pos [N bool [A]],
    margin, pos_share: the share of the classification loss that comes from positive anchors' rows).  cls / reg are differentiable
    w.r.t. classification / regression."""
    assert kind in R.KINDS and cls_kind in CLS_KINDS, (kind, cls_kind)
    anc = anchors.reshape(-1, 4).to(dtype)
    ann = annotations.to(dtype)
    cls, reg = classification.to(dtype), regression.to(dtype)
    N, A, K = cls.shape
    lab = [True] * N if valid is None else [bool(int(v)) for v in valid]
    zero = (cls.sum() + reg.sum()) * 0
    cls_terms, reg_terms, iou_terms, npos, qs, poss, margin = [], [], [], [], [], [], float("inf")
    from_pos = total = 0.0
    for n in range(N):
        if not lab[n]:
            npos.append(0)
            qs.append(torch.zeros(0, dtype=dtype))
            poss.append(torch.zeros(A, dtype=torch.bool))
            continue
        as_n = max_iou_assign(anc, ann[n]) if assign is None else torch.as_tensor(assign[n]).long()
        pos, counted = as_n >= 0, as_n != -2
        p = int(pos.sum())
        npos.append(p)
        poss.append(pos)
        y = torch.zeros(A, K, dtype=dtype)
        if p > 0:
            box = ann[n][as_n[pos]]
            loss, iou, m = R.box_losses(reg[n][pos], anc[pos], box[:, :4], kind)
            margin = min(margin, m)
            q = iou.detach()
            cid = box[:, 4].long()
            hit = (cid >= 0) & (cid < K)                               # a class id outside 0 .. K - 1 matches no k
            y[torch.nonzero(pos)[:, 0][hit], cid[hit]] = q[hit]
            reg_terms.append(loss.sum() / p)
            iou_terms.append(q.sum() / p)
            qs.append(q)
        else:
            reg_terms.append(zero)
            iou_terms.append(torch.zeros((), dtype=dtype))
            qs.append(torch.zeros(0, dtype=dtype))
        l = term(cls[n], y, cls_kind) * counted[:, None].to(dtype)
        cls_terms.append(l.sum() / max(p, 1))
        from_pos += float(l.detach()[pos].sum()) / max(p, 1)
        total += float(l.detach().sum()) / max(p, 1)
    nlab = sum(lab)
    mean = (lambda ts: torch.stack(ts).sum() / nlab) if nlab else (lambda ts: zero)
    return dict(cls=mean(cls_terms), reg=mean(reg_terms), pos_iou=mean(iou_terms).detach(), npos=npos, q=qs, pos=poss, margin=margin,
                pos_share=from_pos / total if total > 0 else 0.0)


# ------------------------------------------------------------------------------------------------------------------------------------
# the inputs the GPU tests run on (tests/test_det_quality_cpu.py measures what float32 alone costs on the same ones)
# ------------------------------------------------------------------------------------------------------------------------------------
def quiet(cls, anchors, annotations):
    """cls with the probabilities of every non-positive anchor (max-IoU assignment) multiplied by 0.05: on the generated inputs the
    background terms are >= 99.99 % of the loss; here the positive anchors' rows carry most of it"""
    anc = anchors.reshape(-1, 4).double()
    out = cls.clone()
    for n in range(cls.shape[0]):
        pos = max_iou_assign(anc, annotations[n].double()) >= 0
        out[n][~pos] = out[n][~pos] * 0.05
    return out


def kat_inputs(z):
    """the recorded KAT inputs (the arrays of loss_kats.npz) with the probabilities test_det_iou_gpu.kats builds: both clamp ends hit"""
    t = lambda k: torch.from_numpy(z[k])
    cls = (t("det/cls") * 4.5).clamp(0, 1)
    cls[0, :50] = 0.0
    cls[0, 50:100] = 1.0
    return dict(cls=cls, reg=t("det/reg"), anc=t("det/anchors").reshape(-1, 4), ann=t("det/ann"))
