"""fp64 numpy restatement of pycocotools COCOeval(gt, dt, 'bbox') evaluate / accumulate / summarize with the default parameters, written
from the rules (no pycocotools).  The oracle of the device evaluator (multitask_hydranet_amd.det_eval); slow (a Python loop per image,
category, area range and detection), like the original.

    GT per (image, category) in annotation order; a GT is ignored when iscrowd or its `area` field is outside the area range (inclusive);
    GTs stably sorted with the non-ignored first.  Detections: area = w * h of the bbox; stable descending score order, first 100 kept.
    IoU = maskApi bbIou in fp64.  Per threshold t, per detection in order: scan the GTs in the sorted order, skip the matched ones, stop at
    the first ignored GT once a non-ignored match exists, skip IoU < current best (starting at min(t, 1 - 1e-10)), else take it (so the
    later GT wins a tie).  dtIg = the matched GT's ignore flag, or (unmatched) the detection's area outside the range.
    accumulate: per (category, area, maxDets): each image's first maxDets detections, concatenated in image order, stable-sorted by
    descending score; tp / fp cumulative sums; rc = tp / npig, pr = tp / (fp + tp + eps); right-to-left envelope;
    q[r] = pr[searchsorted_left(rc, recThrs[r])], 0 past the end; recall = rc[-1] (0 with no detection); npig == 0 leaves -1."""
import numpy as np

IOU_THRS = np.linspace(.5, 0.95, 10)
REC_THRS = np.linspace(.0, 1.00, 101)
MAX_DETS = [1, 10, 100]
AREA_RNG = [[0.0, 1e10], [0.0, 1024.0], [1024.0, 9216.0], [9216.0, 1e10]]


def bb_iou(d, g):
    """maskApi bbIou for xywh boxes d [D,4], g [G,4] -> [D,G]"""
    d = np.asarray(d, dtype=np.float64).reshape(-1, 4)
    g = np.asarray(g, dtype=np.float64).reshape(-1, 4)
    out = np.zeros((len(d), len(g)))
    for j in range(len(g)):
        G = g[j]
        ga = G[2] * G[3]
        for i in range(len(d)):
            D = d[i]
            da = D[2] * D[3]
            w = min(D[2] + D[0], G[2] + G[0]) - max(D[0], G[0])
            if w <= 0:
                continue
            h = min(D[3] + D[1], G[3] + G[1]) - max(D[1], G[1])
            if h <= 0:
                continue
            i_ = w * h
            out[i, j] = i_ / (da + ga - i_)
    return out


def evaluate_img(gts, dts, arng, max_det=100):
    """gts: list of (bbox, area, iscrowd) in annotation order; dts: list of (bbox, score) in result order.  None if both are empty."""
    if not gts and not dts:
        return None
    gt_ig = np.array([1 if (c or a < arng[0] or a > arng[1]) else 0 for _, a, c in gts], dtype=np.int64)
    gind = np.argsort(gt_ig, kind="mergesort")
    gt_ig = gt_ig[gind]
    g_box = [gts[i][0] for i in gind]
    crowd = [gts[i][2] for i in gind]
    dind = np.argsort([-s for _, s in dts], kind="mergesort")[:max_det]
    d_box = [dts[i][0] for i in dind]
    d_score = np.array([dts[i][1] for i in dind], dtype=np.float64)
    T, G, D = len(IOU_THRS), len(g_box), len(d_box)
    ious = bb_iou(d_box, g_box) if (G and D) else np.zeros((D, G))
    gtm = np.zeros((T, G), dtype=bool)
    dtm = np.zeros((T, D), dtype=bool)
    dt_ig = np.zeros((T, D), dtype=bool)
    if G and D:
        for t, thr in enumerate(IOU_THRS):
            for d in range(D):
                iou = min(thr, 1 - 1e-10)
                m = -1
                for g in range(G):
                    if gtm[t, g] and not crowd[g]:
                        continue
                    if m > -1 and gt_ig[m] == 0 and gt_ig[g] == 1:
                        break
                    if ious[d, g] < iou:
                        continue
                    iou = ious[d, g]
                    m = g
                if m == -1:
                    continue
                dt_ig[t, d] = gt_ig[m]
                dtm[t, d] = True
                gtm[t, m] = True
    d_area = np.array([b[2] * b[3] for b in d_box], dtype=np.float64)
    out_rng = (d_area < arng[0]) | (d_area > arng[1])
    dt_ig = dt_ig | (~dtm & out_rng[None, :])
    return dict(dtm=dtm, dtIg=dt_ig, gtIg=gt_ig, scores=d_score)


def coco_eval_ref(gt_ds, results, img_ids=None, max_images=10000):
    """gt_ds: COCO dataset dict; results: list of {image_id, category_id, bbox, score}; img_ids: params.imgIds (default: the first
    max_images GT image ids).  Returns dict(stats, precision [T,R,K,A,M], recall [T,K,A,M]).  Scores are taken as fp32 (the device
    evaluator's comparison; the package's records are fp32 values)."""
    all_ids = [im["id"] for im in gt_ds["images"]]
    gt_set = set(all_ids)
    for r in results:
        if r["image_id"] not in gt_set:
            raise ValueError("Results do not correspond to current coco set")
    if img_ids is None:
        img_ids = all_ids[:max_images]
    img_ids = list(np.unique(img_ids))
    cat_ids = sorted({c["id"] for c in gt_ds["categories"]})
    iset, cset = set(img_ids), set(cat_ids)
    gts, dts = {}, {}
    for a in gt_ds["annotations"]:
        if a["image_id"] in iset and a["category_id"] in cset:
            gts.setdefault((a["image_id"], a["category_id"]), []).append((a["bbox"], a["area"], int(a.get("iscrowd", 0))))
    for r in results:
        if r["image_id"] in iset and r["category_id"] in cset:
            dts.setdefault((r["image_id"], r["category_id"]), []).append((r["bbox"], float(np.float32(r["score"]))))
    T, R, K, A, M = len(IOU_THRS), len(REC_THRS), len(cat_ids), len(AREA_RNG), len(MAX_DETS)
    precision = -np.ones((T, R, K, A, M))
    recall = -np.ones((T, K, A, M))
    for k, c in enumerate(cat_ids):
        for a, arng in enumerate(AREA_RNG):
            E = [evaluate_img(gts.get((i, c), []), dts.get((i, c), []), arng) for i in img_ids]
            E = [e for e in E if e is not None]
            if not E:
                continue
            npig = int(sum(np.count_nonzero(e["gtIg"] == 0) for e in E))
            if npig == 0:
                continue
            for m, md in enumerate(MAX_DETS):
                sc = np.concatenate([e["scores"][:md] for e in E])
                inds = np.argsort(-sc, kind="mergesort")
                dtm = np.concatenate([e["dtm"][:, :md] for e in E], axis=1)[:, inds]
                dig = np.concatenate([e["dtIg"][:, :md] for e in E], axis=1)[:, inds]
                tps = np.logical_and(dtm, np.logical_not(dig))
                fps = np.logical_and(np.logical_not(dtm), np.logical_not(dig))
                tp_sum = np.cumsum(tps, axis=1).astype(np.float64)
                fp_sum = np.cumsum(fps, axis=1).astype(np.float64)
                for t in range(T):
                    tp, fp = tp_sum[t], fp_sum[t]
                    nd = len(tp)
                    rc = tp / npig
                    pr = tp / (fp + tp + np.spacing(1))
                    recall[t, k, a, m] = rc[-1] if nd else 0
                    pr = pr.tolist()
                    for i in range(nd - 1, 0, -1):
                        if pr[i] > pr[i - 1]:
                            pr[i - 1] = pr[i]
                    q = np.zeros(R)
                    for ri, pi in enumerate(np.searchsorted(rc, REC_THRS, side="left")):
                        if pi >= nd:
                            break
                        q[ri] = pr[pi]
                    precision[t, :, k, a, m] = q
    return dict(stats=summarize(precision, recall), precision=precision, recall=recall)


def summarize(precision, recall):
    """COCOeval._summarizeDets"""
    lbl = ["all", "small", "medium", "large"]

    def one(ap, iou=None, area="all", md=100):
        s = precision if ap else recall
        if iou is not None:
            s = s[np.where(iou == IOU_THRS)[0]]
        s = s[..., lbl.index(area), MAX_DETS.index(md)]
        return -1.0 if len(s[s > -1]) == 0 else float(np.mean(s[s > -1]))
    return np.array([one(1), one(1, .5), one(1, .75), one(1, area="small"), one(1, area="medium"), one(1, area="large"),
                     one(0, md=1), one(0, md=10), one(0), one(0, area="small"), one(0, area="medium"), one(0, area="large")])


def synthetic_set(n_images, seed=0, width=1920, height=1080, max_gt=40, dets_per_image=100, n_cat=9):
    """a validation set in COCO form: (GT dataset dict, result records).  Per image 0..max_gt GTs over n_cat classes with integer
    boxes whose areas straddle 32^2 and 96^2 (some exactly 1024 / 9216), ~dets_per_image detections: jittered GTs (some cut to an exact
    IoU of 0.5 or 0.75), false positives and off-class boxes, fp32 scores quantised to 1/64 so ties occur; empty images, images with GTs
    and no detections, and a category without GT."""
    rng = np.random.default_rng(seed)
    cats = [{"id": i + 1, "name": "c%d" % i} for i in range(n_cat)]
    images, anns, res = [], [], []
    aid = 0
    for i in range(n_images):
        iid = i + 1
        images.append({"id": iid, "width": width, "height": height})
        kind = (i + seed) % 11
        ng = 0 if kind == 0 else int(rng.integers(0, max_gt + 1))
        side = np.exp(rng.uniform(np.log(8), np.log(300), ng))
        gts = []
        for j in range(ng):
            w = int(max(1, round(side[j] * rng.uniform(0.6, 1.6))))
            h = int(max(1, round(side[j] * rng.uniform(0.6, 1.6))))
            if j % 13 == 5:
                w, h = 32, 32
            elif j % 13 == 9:
                w, h = 96, 96
            x, y = float(rng.integers(0, width - w)), float(rng.integers(0, height - h))
            c = int(rng.integers(1, n_cat))              # class n_cat never has GT
            aid += 1
            anns.append({"id": aid, "image_id": iid, "category_id": c, "bbox": [x, y, w, h], "area": w * h, "iscrowd": 0})
            gts.append((x, y, w, h, c))
        if kind == 1:
            continue                                     # GTs but no detection
        nd = int(rng.integers(dets_per_image // 2, dets_per_image + 1)) if kind != 0 else int(rng.integers(0, 5))
        for j in range(nd):
            u = rng.uniform()
            if gts and u < 0.55:
                x, y, w, h, c = gts[int(rng.integers(0, len(gts)))]
                v = rng.uniform()
                if v < 0.1:
                    w = w * 0.5                          # IoU exactly 0.5 (half the box, same corner)
                elif v < 0.2:
                    w = w * 0.75                         # exactly 0.75
                elif v < 0.3:
                    pass                                 # the GT itself
                else:
                    s = 0.15 * np.sqrt(w * h)
                    x, y = x + rng.normal(0, s), y + rng.normal(0, s)
                    w, h = max(1.0, w + rng.normal(0, s)), max(1.0, h + rng.normal(0, s))
                if rng.uniform() < 0.05:
                    c = int(rng.integers(1, n_cat + 1))
            else:
                w = float(np.exp(rng.uniform(np.log(4), np.log(400))))
                h = float(np.exp(rng.uniform(np.log(4), np.log(400))))
                if rng.uniform() < 0.05:
                    w, h = 32.0, 32.0
                x, y = float(rng.uniform(0, width - w)), float(rng.uniform(0, height - h))
                c = int(rng.integers(1, n_cat + 1))
            # the json holds fp32 values (coco_json.detections_to_coco): x, y, w, h and the score
            b = np.asarray([x, y, w, h], dtype=np.float32)
            score = np.float32(np.floor(rng.uniform(0.05, 1.0) * 64) / 64)
            res.append({"image_id": iid, "category_id": c, "bbox": b.tolist(), "score": float(score)})
    return {"images": images, "annotations": anns, "categories": cats}, res
