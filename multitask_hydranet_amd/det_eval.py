"""COCO box mAP of the detection validation on the device: pycocotools' COCOeval(coco_gt, coco_dt, 'bbox') with
`params.imgIds = coco_gt.getImgIds()[:cfgs["detection"]["max_images"]]` and the default parameters, evaluate() + accumulate() + summarize(),
as head_detect/detect_eval.py:_eval runs it at model/train.py:416-426.  pycocotools is not needed.

The rules that decide the numbers (kernels: csrc/hn_coco.hip):
  * iouThrs = linspace(.5, .95, 10), recThrs = linspace(0, 1, 101) (fp64, from numpy, passed to the device as they are); maxDets 1, 10,
    100; area ranges all [0, 1e10], small [0, 32^2], medium [32^2, 96^2], large [96^2, 1e10], inclusive; categories = sorted ids of the
    GT's `categories`, detections of other categories dropped; images = sorted unique ids (COCOeval's np.unique of params.imgIds).
  * GT area = the annotation's `area` field; detection area = w * h of its bbox; IoU = maskApi bbIou on the bboxes in fp64.
  * evaluateImg, accumulate and summarize exactly as COCOeval (the kernels' header comment restates them); `stats` are the 12 numbers
    in COCOeval's order, each the mean of the entries > -1, or -1.
  * Scores are compared as fp32: the post-process produces fp32 scores, so the package's own records are unchanged; a results file with
    scores that are not fp32 values is rounded to the nearest fp32 first.
  * Image ids follow the reference: detections of batch b, image i get id b * batch_size_valid + i + 1 (HydraTrainer.valid), GT ids come
    from the GT json, where gen_coco_label skips images without annotations -- so the two can be misaligned exactly as in the reference.
    A detection whose image id is not a GT image raises ValueError (COCO.loadRes' assertion); ids in the GT but outside the evaluated
    images are ignored.  With no detection at all the reference skips the evaluation: compute() returns None.
  * iscrowd GTs (never written by the reference's GT writer) are rejected with ValueError; crowd IoU is not implemented.  An image's
    detections must arrive in one update() (a repeated image raises ValueError).
"""
from __future__ import annotations

import json
from typing import List, Optional, Sequence

import numpy as np

IOU_THRS = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
REC_THRS = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
MAX_DETS = [1, 10, 100]
AREA_RNG = [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]
AREA_LBL = ["all", "small", "medium", "large"]
MAX_DET_CELL = 100          # evaluateImg's maxDet (p.maxDets[-1]): detections kept per (image, category)
_REC_INTS = 8               # one record: {score bits, image order * 128 + rank, category, 0, bits per area range}


def load_ground_truth(coco_gt) -> dict:
    """the GT dataset dict from a dict (coco_json.coco_ground_truth), a path to gt_bbox_results.json or a pycocotools COCO object"""
    if isinstance(coco_gt, dict):
        return coco_gt
    if isinstance(coco_gt, str):
        with open(coco_gt) as f:
            return json.load(f)
    if hasattr(coco_gt, "dataset"):
        return coco_gt.dataset
    raise TypeError("coco_gt: a COCO dataset dict, a path to a GT json or an object with .dataset")


def summarize_stats(precision: np.ndarray, recall: np.ndarray) -> np.ndarray:
    """COCOeval._summarizeDets on precision [T,R,K,A,M] and recall [T,K,A,M]"""
    def one(ap, iou=None, area="all", md=100):
        s = precision if ap else recall
        if iou is not None:
            s = s[np.where(iou == IOU_THRS)[0]]
        a, m = AREA_LBL.index(area), MAX_DETS.index(md)
        s = s[:, :, :, a, m] if ap else s[:, :, a, m]
        return -1.0 if len(s[s > -1]) == 0 else float(np.mean(s[s > -1]))
    return np.array([one(1), one(1, .5), one(1, .75), one(1, area="small"), one(1, area="medium"), one(1, area="large"),
                     one(0, md=1), one(0, md=10), one(0), one(0, area="small"), one(0, area="medium"), one(0, area="large")])


def summary_lines(stats: Sequence[float]) -> List[str]:
    """the 12 lines COCOeval.summarize() prints"""
    rows = [(1, None, "all", 100), (1, .5, "all", 100), (1, .75, "all", 100), (1, None, "small", 100), (1, None, "medium", 100),
            (1, None, "large", 100), (0, None, "all", 1), (0, None, "all", 10), (0, None, "all", 100), (0, None, "small", 100),
            (0, None, "medium", 100), (0, None, "large", 100)]
    out = []
    for (ap, iou, area, md), v in zip(rows, stats):
        iou_s = "{:0.2f}:{:0.2f}".format(IOU_THRS[0], IOU_THRS[-1]) if iou is None else "{:0.2f}".format(iou)
        out.append(" {:<18} {} @[ IoU={:<9} | area={:>6s} | maxDets={:>3d} ] = {:0.3f}".format(
            "Average Precision" if ap else "Average Recall", "(AP)" if ap else "(AR)", iou_s, area, md, v))
    return out


class CocoBoxEvaluator:
    """Streaming COCO bbox evaluation on the device.  coco_gt: the dataset dict of coco_json.coco_ground_truth, a path to
    gt_bbox_results.json (or a pycocotools COCO object); img_ids: COCOeval's params.imgIds (default: the GT's first `max_images` image ids
    in file order, as model/train.py:185).  update() takes the per-image prediction dicts of HydraTrainer.valid after invert_affine;
    compute() returns dict(stats, precision, recall) (numpy float64), or None when no detection was given."""

    def __init__(self, coco_gt, img_ids=None, max_images: int = 10000, device=None):
        import torch
        from . import _lib
        ds = load_ground_truth(coco_gt)
        self.device = torch.device(device if device is not None else "cuda")
        self.cat_ids = sorted({int(c["id"]) for c in ds["categories"]})
        gt_img_ids = list(dict.fromkeys(int(im["id"]) for im in ds["images"]))       # COCO.getImgIds(): dict insertion order
        if img_ids is None:
            img_ids = gt_img_ids[:max_images]
        self.img_ids = np.unique(np.asarray(list(img_ids), dtype=np.int64))
        self._gt_ids = np.unique(np.asarray(gt_img_ids, dtype=np.int64))
        K, I = len(self.cat_ids), len(self.img_ids)
        if K == 0:
            raise ValueError("the ground truth has no category")
        if I * 128 >= 2 ** 31:
            raise ValueError("too many images for the record sequence (image order * 128 + rank must fit in 31 bits)")
        anns = ds["annotations"]
        if any(a.get("iscrowd", 0) for a in anns):
            raise ValueError("iscrowd ground truth is not supported (the reference's GT writer never emits it; crowd IoU is out of scope)")
        # GT cells in annotation order: cell = image order * K + category index
        a_img = np.asarray([int(a["image_id"]) for a in anns], dtype=np.int64)
        a_cat = np.asarray([int(a["category_id"]) for a in anns], dtype=np.int64)
        io, ko = self._img_order(a_img), self._cat_index(a_cat)
        keep = (io >= 0) & (ko >= 0)
        box = np.zeros((len(anns), 5), dtype=np.float64)
        if anns:
            box[:, :4] = np.asarray([a["bbox"] for a in anns], dtype=np.float64).reshape(-1, 4)
            box[:, 4] = np.asarray([a["area"] for a in anns], dtype=np.float64)
        cell = (io * K + ko)[keep]
        order = np.argsort(cell, kind="stable")
        self.gt = gt = np.ascontiguousarray(box[keep][order])          # [G][5]: x, y, w, h, area
        self.gt_off = np.zeros(I * K + 1, dtype=np.int32)
        np.cumsum(np.bincount(cell, minlength=I * K), out=self.gt_off[1:])
        # npig per (category, area range): COCOeval counts the non-ignored GTs of every evaluated image, with or without detections
        gk = ko[keep][order]
        self.npig = np.zeros((K, 4), dtype=np.int32)
        for a, (lo, hi) in enumerate(AREA_RNG):
            inr = (gt[:, 4] >= lo) & (gt[:, 4] <= hi)
            self.npig[:, a] = np.bincount(gk[inr], minlength=K)
        self.n_gt = len(gt)
        prm = np.concatenate([np.minimum(IOU_THRS, 1 - 1e-10), np.asarray(AREA_RNG, dtype=np.float64).reshape(-1)])
        self._lib = _lib.lib()
        self._gt_off_d = torch.from_numpy(self.gt_off).to(self.device)
        self._gt_d = torch.from_numpy(gt.reshape(-1) if len(gt) else np.zeros(5)).to(self.device)
        self._prm_d = torch.from_numpy(prm).to(self.device)
        self._rthr_d = torch.from_numpy(REC_THRS.copy()).to(self.device)
        self._gtm_ws = torch.empty(int(self._lib.query("hn_coco_match_ws_bytes", self.n_gt)), dtype=torch.uint8, device=self.device)
        self.reset()

    def reset(self):
        self._chunks = []              # per update: (records [n, 8] int32 on the device, kept records per category)
        self._n_raw = 0                # detections given to update(), before any filter
        self._seen = np.zeros(len(self.img_ids), dtype=bool)

    @staticmethod
    def _index_in(sorted_ids, ids):
        """position of every id in the sorted array `sorted_ids`, -1 where it is absent"""
        if len(sorted_ids) == 0:
            return np.full(len(ids), -1, dtype=np.int64)
        pos = np.minimum(np.searchsorted(sorted_ids, ids), len(sorted_ids) - 1)
        return np.where(sorted_ids[pos] == ids, pos, -1)

    def _img_order(self, ids):
        return self._index_in(self.img_ids, ids)

    def _cat_index(self, cats):
        return self._index_in(np.asarray(self.cat_ids, dtype=np.int64), cats)

    def update(self, preds: Sequence[dict], first_image_id: int):
        """preds: per-image dicts {rois [n,4] x1,y1,x2,y2 (source-image pixels), class_ids [n], scores [n]} of one validation batch; image
        k gets id first_image_id + k.  x,y,w,h are formed in fp32 as coco_json.detections_to_coco does, so the device sees the values the
        results json records."""
        ids, cats, boxes, scores = [], [], [], []
        for k, pr in enumerate(preds):
            rois = np.asarray(pr["rois"], dtype=np.float32)
            if rois.ndim != 2 or rois.shape[0] == 0:
                continue
            rois = rois.copy()
            rois[:, 2] -= rois[:, 0]
            rois[:, 3] -= rois[:, 1]
            boxes.append(rois.astype(np.float64))
            ids.append(np.full(len(rois), first_image_id + k, dtype=np.int64))
            cats.append(np.asarray(pr["class_ids"], dtype=np.int64).reshape(-1) + 1)
            scores.append(np.asarray(pr["scores"], dtype=np.float32).reshape(-1))
        if not ids:
            return
        self.update_records(np.concatenate(ids), np.concatenate(cats), np.concatenate(boxes), np.concatenate(scores))

    def update_records(self, image_ids, category_ids, bboxes, scores):
        """detections in COCO result form: image_id [n], category_id [n], bbox [n, 4] x,y,w,h (fp64), score [n] (compared as fp32); one
        host buffer, one copy to the device, one match launch"""
        import torch
        image_ids = np.asarray(image_ids, dtype=np.int64).reshape(-1)
        n = len(image_ids)
        if n == 0:
            return
        category_ids = np.asarray(category_ids, dtype=np.int64).reshape(-1)
        bboxes = np.asarray(bboxes, dtype=np.float64).reshape(n, 4)
        scores = np.asarray(scores, dtype=np.float32).reshape(-1).astype(np.float64)
        unknown = ~np.isin(image_ids, self._gt_ids)
        if unknown.any():
            raise ValueError("Results do not correspond to current coco set: image id %d is not a ground-truth image" % image_ids[unknown][0])
        self._n_raw += n
        io, ko = self._img_order(image_ids), self._cat_index(category_ids)
        keep = (io >= 0) & (ko >= 0)
        if not keep.any():
            return
        imgs = np.unique(io[keep])
        if self._seen[imgs].any():
            raise ValueError("image id %d was already given to an earlier update()" % self.img_ids[imgs[self._seen[imgs]][0]])
        self._seen[imgs] = True
        K = len(self.cat_ids)
        cell = (io * K + ko)[keep]
        order = np.argsort(cell, kind="stable")                 # the cell's detections in input order (the kernel's stable rank)
        dets = np.empty((len(order), 5), dtype=np.float64)
        dets[:, :4] = bboxes[keep][order]
        dets[:, 4] = scores[keep][order]
        ucell, first, count = np.unique(cell[order], return_index=True, return_counts=True)
        kept = np.minimum(count, MAX_DET_CELL)
        rec0 = np.zeros(len(ucell), dtype=np.int64)
        np.cumsum(kept[:-1], out=rec0[1:])
        cells = np.stack([ucell, first, count, rec0], 1).astype(np.int32)
        n_rec = int(kept.sum())
        buf = np.concatenate([cells.reshape(-1).view(np.uint8), dets.reshape(-1).view(np.uint8)])     # cells first: 16-byte rows
        dev = torch.from_numpy(buf).to(self.device)
        rec = torch.empty((n_rec, _REC_INTS), dtype=torch.int32, device=self.device)
        base = dev.data_ptr()
        self._lib.call("hn_coco_match", base, len(ucell), base + cells.nbytes, self._gt_off_d.data_ptr(), self._gt_d.data_ptr(),
                       self._prm_d.data_ptr(), K, len(IOU_THRS), self._gtm_ws.data_ptr(), rec.data_ptr())
        per_cat = np.bincount(ucell % K, weights=kept, minlength=K).astype(np.int64)
        self._chunks.append((rec, per_cat))

    def compute(self) -> Optional[dict]:
        """dict(stats [12], precision [T,R,K,A,M], recall [T,K,A,M]) as numpy float64; None when no detection was given"""
        import torch
        if self._n_raw == 0:
            return None
        K, T, R, M = len(self.cat_ids), len(IOU_THRS), len(REC_THRS), len(MAX_DETS)
        recs = [c[0] for c in self._chunks]
        rec = torch.cat(recs) if len(recs) > 1 else (recs[0] if recs else torch.zeros((0, _REC_INTS), dtype=torch.int32, device=self.device))
        N = rec.shape[0]
        per_cat = sum((c[1] for c in self._chunks), np.zeros(K, dtype=np.int64))
        cat_start = np.zeros(K + 1, dtype=np.int64)
        np.cumsum(per_cat, out=cat_start[1:])
        iprm = np.concatenate([cat_start, self.npig.reshape(-1), np.asarray(MAX_DETS)]).astype(np.int32)
        iprm_d = torch.from_numpy(iprm).to(self.device)
        ws = torch.empty(int(self._lib.query("hn_coco_accumulate_ws_bytes", N)), dtype=torch.uint8, device=self.device)
        precision = torch.empty((T, R, K, 4, M), dtype=torch.float64, device=self.device)
        recall = torch.empty((T, K, 4, M), dtype=torch.float64, device=self.device)
        seq_bits = max(int(len(self.img_ids) * 128 - 1).bit_length(), 1)
        self._lib.call("hn_coco_accumulate", rec.data_ptr() if N else 0, N, K, seq_bits, iprm_d.data_ptr(), self._rthr_d.data_ptr(), T, R,
                       M, ws.data_ptr(), precision.data_ptr(), recall.data_ptr())
        p, r = precision.cpu().numpy(), recall.cpu().numpy()
        self.result = dict(stats=summarize_stats(p, r), precision=p, recall=r)
        return self.result

    def summary(self) -> List[str]:
        """the 12 lines of COCOeval.summarize() for the last compute()"""
        res = getattr(self, "result", None)
        if res is None:
            res = self.compute()
        if res is None:
            return []
        return summary_lines(res["stats"])


def _eval(coco_gt, image_ids, pred_json_path):
    """head_detect/detect_eval.py:_eval on the device: the results json through the same packer and kernels, the summary printed;
    returns the 12 stats (the reference returns nothing), or None when the file holds no detection"""
    print(pred_json_path)
    with open(pred_json_path) as f:
        res = json.load(f)
    print("BBox")
    ev = CocoBoxEvaluator(coco_gt, img_ids=image_ids)
    if res:
        ev.update_records([r["image_id"] for r in res], [r["category_id"] for r in res], [r["bbox"] for r in res],
                          [r["score"] for r in res])
    out = ev.compute()
    if out is None:
        return None
    for line in summary_lines(out["stats"]):
        print(line)
    return out["stats"]
