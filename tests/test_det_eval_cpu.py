"""CPU: the fp64 COCOeval restatement (tests/coco_eval_ref.py) pinned by hand-derived cases, and the host side of
multitask_hydranet_amd.det_eval (GT packing, image-id rules, the summary format); no kernel is launched here.

pr = tp / (fp + tp + eps) with eps = 2^-52: a precision of "1" is 1 / (1 + 2^-52) = 1 - 2^-52 (P1 below), so hand values are compared
at 1e-12.  The same cases run through the kernels in tests/test_det_eval_gpu.py."""
import numpy as np
import pytest

from tests.coco_eval_ref import coco_eval_ref

P1 = 1.0 / (1.0 + 2.0 ** -52)
LARGE = 10000          # area of a 100 x 100 box


def dataset(images):
    """images: {image_id: [(x, y, w, h, category[, area]), ...]} -> COCO GT dict with categories 1..9"""
    anns, aid = [], 0
    for iid, boxes in images.items():
        for b in boxes:
            aid += 1
            area = b[5] if len(b) > 5 else int(b[2] * b[3])
            anns.append({"id": aid, "image_id": iid, "category_id": b[4], "bbox": [float(v) for v in b[:4]], "area": area, "iscrowd": 0})
    return {"images": [{"id": i} for i in images], "annotations": anns, "categories": [{"id": c} for c in range(1, 10)]}


def det(iid, cat, box, score):
    return {"image_id": iid, "category_id": cat, "bbox": [float(v) for v in box], "score": float(score)}


def _perfect():
    # one GT, one exact detection: every threshold matches; rc = 1, pr = P1 at every recall threshold; only 'all' and 'large' have GT
    return dataset({1: [(10, 10, 100, 100, 1)]}), [det(1, 1, (10, 10, 100, 100), .9)]


def _check_perfect(r):
    assert np.allclose(r["stats"], [P1, P1, P1, -1, -1, P1, 1, 1, 1, -1, -1, 1], rtol=0, atol=1e-12)
    assert (r["precision"][:, :, 0, 0, :] == P1).all() and (r["recall"][:, 0, 0, :] == 1).all()
    assert (r["precision"][:, :, 1:] == -1).all()                       # categories 2..9: no GT


def _tp_fp_tp():
    # GTs A, B; detections A (.9), a miss (.8), B (.7): tp = 1,1,2, fp = 0,1,1 -> rc = .5,.5,1, pr = P1, .5, 2/3; envelope P1, 2/3, 2/3;
    # recall thresholds 0..0.50 (51 of them) read index 0 -> P1, 0.51..1 (50) read index 2 -> 2/3: AP = (51 P1 + 50 * 2/3) / 101
    return (dataset({1: [(0, 0, 100, 100, 1), (200, 0, 100, 100, 1)]}),
            [det(1, 1, (0, 0, 100, 100), .9), det(1, 1, (400, 0, 100, 100), .8), det(1, 1, (200, 0, 100, 100), .7)])


def _check_tp_fp_tp(r):
    ap = (51 * P1 + 50 * (2 / 3)) / 101
    assert abs(r["stats"][0] - ap) < 1e-12 and abs(r["stats"][1] - ap) < 1e-12 and r["stats"][8] == 1
    assert r["recall"][0, 0, 0, 0] == 0.5                                # maxDets 1: only the first detection (A)


def _iou_half():
    # det [0,0,50,100] on GT [0,0,100,100]: i = 5000, u = 5000 + 10000 - 5000 = 10000, IoU = 0.5 exactly: matches at .50 only
    return dataset({1: [(0, 0, 100, 100, 1)]}), [det(1, 1, (0, 0, 50, 100), .9)]


def _check_iou_half(r):
    assert (r["precision"][0, :, 0, 0, 2] == P1).all() and (r["precision"][1:, :, 0, 0, 2] == 0).all()
    assert r["recall"][0, 0, 0, 2] == 1 and (r["recall"][1:, 0, 0, 2] == 0).all()
    assert abs(r["stats"][1] - P1) < 1e-12 and r["stats"][2] == 0 and abs(r["stats"][0] - P1 / 10) < 1e-12


def _iou_tie():
    # G1 [0,0,100,100], G2 [50,0,100,100]; det1 [25,0,100,100] (.9) has IoU 7500 / 12500 = fl(0.6) with both: the LATER GT (G2) wins at
    # t = .50, .55 and linspace[2] (which is fl(0.6) itself), so det2 = G1 (.8) still finds G1 -> recall 1.  From t = .65 on det1 is
    # unmatched and det2 -> G1: recall .5.  (Had det1 taken G1, det2 would have IoU 1/3 with G2: recall .5 at every threshold.)
    return (dataset({1: [(0, 0, 100, 100, 1), (50, 0, 100, 100, 1)]}),
            [det(1, 1, (25, 0, 100, 100), .9), det(1, 1, (0, 0, 100, 100), .8)])


def _check_iou_tie(r):
    assert list(r["recall"][:, 0, 0, 2]) == [1, 1, 1] + [.5] * 7


def _ignored_gt():
    # a large GT (10000) and a small one (400, 20 x 20); det1 (.9) on the large GT, det2 (.5) on the small one.  'small': the large GT
    # is ignored, so det1 is ignored (neither tp nor fp): [ig, tp] -> rc 0, 1, pr 0, P1 -> envelope P1, P1 -> AP small = P1.
    # (Counted as a false positive it would give pr .5 at rc 1: AP .5.)
    return (dataset({1: [(0, 0, 100, 100, 1), (300, 300, 20, 20, 1)]}),
            [det(1, 1, (0, 0, 100, 100), .9), det(1, 1, (300, 300, 20, 20), .5)])


def _check_ignored_gt(r):
    assert abs(r["stats"][3] - P1) < 1e-12 and r["stats"][9] == 1
    assert abs(r["stats"][5] - P1) < 1e-12                               # 'large': det2 is unmatched and its area 400 is out of range


def _area_1024():
    # a 32 x 32 GT (area 1024) and its exact detection: inside [0, 1024] and [1024, 9216] (inclusive bounds), not large
    return dataset({1: [(5, 5, 32, 32, 1)]}), [det(1, 1, (5, 5, 32, 32), .9)]


def _check_area_1024(r):
    assert abs(r["stats"][3] - P1) < 1e-12 and abs(r["stats"][4] - P1) < 1e-12 and r["stats"][5] == -1
    assert r["stats"][9] == 1 and r["stats"][10] == 1 and r["stats"][11] == -1


def _max_dets():
    # 12 separate GTs, 12 exact detections in descending score: recall@1 = 1/12, @10 = 10/12, @100 = 1
    gts = [(150 * (j % 6), 150 * (j // 6), 100, 100, 1) for j in range(12)]
    return dataset({1: gts}), [det(1, 1, g[:4], 0.95 - 0.01 * j) for j, g in enumerate(gts)]


def _check_max_dets(r):
    assert abs(r["stats"][6] - 1 / 12) < 1e-12 and abs(r["stats"][7] - 10 / 12) < 1e-12 and r["stats"][8] == 1


def _over_100():
    # 150 detections per cell; category 1's exact match has the 100th score (rank 99: kept), category 2's the 101st (rank 100: dropped)
    g = {1: [(0, 0, 100, 100, 1), (0, 0, 100, 100, 2)]}
    res = []
    for c in (1, 2):
        hit = 99 if c == 1 else 100
        for j in range(150):
            s = 1.0 - j / 256
            res.append(det(1, c, (0, 0, 100, 100) if j == hit else (200 + 5 * j, 200, 10, 10), s))
    return dataset(g), res


def _check_over_100(r):
    assert (r["recall"][:, 0, 0, 2] == 1).all() and (r["recall"][:, 0, 0, 1] == 0).all()
    assert (r["recall"][:, 1, 0, 2] == 0).all()


def _no_gt_class():
    # category 1 perfect; detections of category 2, which has no GT: npig = 0 -> -1, left out of every mean
    return dataset({1: [(10, 10, 100, 100, 1)]}), [det(1, 1, (10, 10, 100, 100), .9), det(1, 2, (300, 300, 50, 50), .95)]


def _check_no_gt_class(r):
    assert abs(r["stats"][0] - P1) < 1e-12 and r["stats"][8] == 1
    assert (r["precision"][:, :, 1] == -1).all() and (r["recall"][:, 1] == -1).all()


def _tied_scores():
    # equal scores in two images keep image order: image 1 a miss, image 2 a hit -> [fp, tp]: rc 0, .5, pr 0, .5 -> AP = 51 * .5 / 101
    # (the records list image 2 first; the concatenation follows the sorted image ids.  [tp, fp] would give 51 * P1 / 101)
    return (dataset({1: [(0, 0, 100, 100, 1)], 2: [(0, 0, 100, 100, 1)]}),
            [det(2, 1, (0, 0, 100, 100), .5), det(1, 1, (500, 500, 100, 100), .5)])


def _check_tied_scores(r):
    assert abs(r["stats"][0] - 25.5 / 101) < 1e-12


CASES = {"perfect": (_perfect, _check_perfect), "tp_fp_tp": (_tp_fp_tp, _check_tp_fp_tp), "iou_half": (_iou_half, _check_iou_half),
         "iou_tie": (_iou_tie, _check_iou_tie), "ignored_gt": (_ignored_gt, _check_ignored_gt), "area_1024": (_area_1024, _check_area_1024),
         "max_dets": (_max_dets, _check_max_dets), "over_100": (_over_100, _check_over_100), "no_gt_class": (_no_gt_class, _check_no_gt_class),
         "tied_scores": (_tied_scores, _check_tied_scores)}


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_hand_cases(name):
    make, check = CASES[name]
    gt, res = make()
    check(coco_eval_ref(gt, res))


def test_restatement_against_pycocotools():
    pytest.importorskip("pycocotools")
    import contextlib
    import io
    from pycocotools.coco import COCO
    from pycocotools.cocoeval import COCOeval
    from tests.coco_eval_ref import synthetic_set
    for n, seed in ((1, 0), (37, 1), (120, 2)):
        gt, res = synthetic_set(n, seed, dets_per_image=30)
        with contextlib.redirect_stdout(io.StringIO()):
            cg = COCO()
            cg.dataset = gt
            cg.createIndex()
            ev = COCOeval(cg, cg.loadRes(res), "bbox")
            ev.evaluate()
            ev.accumulate()
            ev.summarize()
        r = coco_eval_ref(gt, res)
        assert np.array_equal(r["precision"], ev.eval["precision"]) and np.array_equal(r["recall"], ev.eval["recall"])
        assert np.allclose(r["stats"], ev.stats, rtol=0, atol=1e-12)


# ---- host side of det_eval (the library is loaded, nothing is launched) ----

@pytest.fixture(scope="module")
def det_eval():
    import __graft_entry__ as g
    g.build()
    from multitask_hydranet_amd import det_eval
    return det_eval


def test_gt_packing_csr(det_eval):
    from multitask_hydranet_amd.coco_json import coco_ground_truth
    ds = coco_ground_truth([
        {"file_name": "a.jpg", "height": 1080, "width": 1920, "annos": ["10,20,110.7,70,3", "5,5,50,50,1", "0,0,40,40,3"]},
        {"file_name": "b.jpg", "height": 1080, "width": 1920, "annos": []},                     # skipped: takes no id
        {"file_name": "c.jpg", "height": 1080, "width": 1920, "annos": ["1.5,2.5,33.5,34.5,9"]}])
    ev = det_eval.CocoBoxEvaluator(ds, device="cpu")
    assert list(ev.img_ids) == [1, 2] and ev.cat_ids == list(range(1, 10))
    K = 9
    off = ev.gt_off
    assert len(off) == 2 * K + 1 and off[-1] == 4
    # image 1 (order 0): category 1 (index 0) one GT, category 3 (index 2) two GTs in annotation order; image 2: category 9 one GT
    assert off[1] - off[0] == 1 and off[3] - off[2] == 2 and off[K + 9] - off[K + 8] == 1
    assert ev.gt[off[2]].tolist() == [10.0, 20.0, 100.0, 50.0, 5000.0]                        # wid = int(100.7) as gen_val_json.py:80
    assert ev.gt[off[2] + 1].tolist() == [0.0, 0.0, 40.0, 40.0, 1600.0]
    assert ev.gt[off[K + 8]].tolist() == [1.5, 2.5, 32.0, 32.0, 1024.0]
    # non-ignored GT counts per (category, area): 1024 is both small and medium
    assert ev.npig[8].tolist() == [1, 1, 1, 0] and ev.npig[2].tolist() == [2, 0, 2, 0] and ev.npig[0].tolist() == [1, 0, 1, 0]


def test_unknown_image_id_and_max_images(det_eval):
    gt, _ = _tp_fp_tp()
    gt["images"] += [{"id": 2}, {"id": 3}]
    ev = det_eval.CocoBoxEvaluator(gt, max_images=2, device="cpu")
    assert list(ev.img_ids) == [1, 2]
    with pytest.raises(ValueError, match="not a ground-truth image"):
        ev.update_records([1, 7], [1, 1], [[0, 0, 1, 1]] * 2, [.5, .5])
    with pytest.raises(ValueError, match="not a ground-truth image"):
        ev.update([{"rois": np.zeros((1, 4), np.float32), "class_ids": np.zeros(1), "scores": np.ones(1, np.float32)}] * 4, 1)
    ev.update_records([3], [1], [[0, 0, 1, 1]], [.5])          # image 3 is a GT image beyond max_images: ignored, nothing launched
    assert ev._n_raw == 1 and ev._chunks == []
    assert det_eval.CocoBoxEvaluator(gt, img_ids=[3, 1, 3], device="cpu").img_ids.tolist() == [1, 3]


def test_iscrowd_rejected(det_eval):
    gt, _ = _perfect()
    gt["annotations"][0]["iscrowd"] = 1
    with pytest.raises(ValueError, match="iscrowd"):
        det_eval.CocoBoxEvaluator(gt, device="cpu")


def test_summary_format(det_eval):
    lines = det_eval.summary_lines([0.5, 0.25, -1, 0, 0, 0, 0.125, 0, 0, 0, 0, 1])
    assert lines[0] == " Average Precision  (AP) @[ IoU=0.50:0.95 | area=   all | maxDets=100 ] = 0.500"
    assert lines[2] == " Average Precision  (AP) @[ IoU=0.75      | area=   all | maxDets=100 ] = -1.000"
    assert lines[6] == " Average Recall     (AR) @[ IoU=0.50:0.95 | area=   all | maxDets=  1 ] = 0.125"
    assert lines[11] == " Average Recall     (AR) @[ IoU=0.50:0.95 | area= large | maxDets=100 ] = 1.000"
    assert det_eval.IOU_THRS[8] == 0.8999999999999999 and det_eval.REC_THRS[57] == np.linspace(0, 1, 101)[57]
