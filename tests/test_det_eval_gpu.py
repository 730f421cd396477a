"""GPU: the COCO box mAP kernels (hn_coco.hip through det_eval.CocoBoxEvaluator) against the fp64 restatement (tests/coco_eval_ref.py):
the hand cases of tests/test_det_eval_cpu.py, randomised sets of 1, 37 and 500 images (empty images, GTs without detections, tied
quantised scores, exact-threshold IoUs, boundary areas) with precision and recall bitwise equal and stats within 1e-12, streaming in
batches, bitwise determinism, and a cell with more GTs than the match kernel keeps in LDS (its global-memory path)."""
import numpy as np
import pytest
import torch

from tests.coco_eval_ref import coco_eval_ref, synthetic_set
from tests.test_det_eval_cpu import CASES, dataset, det

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def E():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    import __graft_entry__ as g
    g.build()
    from multitask_hydranet_amd import det_eval
    return det_eval


def _records(res):
    return ([r["image_id"] for r in res], [r["category_id"] for r in res], [r["bbox"] for r in res], [r["score"] for r in res])


def _device(E, gt, res, batches=None):
    ev = E.CocoBoxEvaluator(gt, device="cuda:0")
    if batches is None:
        ev.update_records(*_records(res))
    else:                                     # stream: every image's records in one update, `batches` images per update
        ids = sorted({r["image_id"] for r in res})
        for b in range(0, len(ids), batches):
            sel = set(ids[b:b + batches])
            ev.update_records(*_records([r for r in res if r["image_id"] in sel]))
    return ev.compute()


def _same(a, b):
    assert np.array_equal(a["precision"], b["precision"]), np.argwhere(a["precision"] != b["precision"])[:5]
    assert np.array_equal(a["recall"], b["recall"]), np.argwhere(a["recall"] != b["recall"])[:5]
    assert np.allclose(a["stats"], b["stats"], rtol=0, atol=1e-12)


@pytest.mark.parametrize("name", sorted(CASES))
def test_hand_cases_on_device(E, name):
    make, check = CASES[name]
    gt, res = make()
    got = _device(E, gt, res)
    check(got)
    _same(got, coco_eval_ref(gt, res))


@pytest.fixture(scope="module")
def sets():
    out = {}
    for n, seed in ((1, 3), (37, 4), (500, 5)):
        gt, res = synthetic_set(n, seed)
        out[n] = (gt, res, coco_eval_ref(gt, res))
    return out


@pytest.mark.parametrize("n", [1, 37, 500])
def test_random_sets_bitwise(E, sets, n):
    gt, res, ref = sets[n]
    got = _device(E, gt, res)
    _same(got, ref)
    assert (ref["precision"] > -1).any() and ref["stats"][0] > 0


@pytest.mark.parametrize("batch", [1, 7, 16])
def test_streaming_equals_one_update(E, sets, batch):
    gt, res, ref = sets[37]
    one = _device(E, gt, res)
    got = _device(E, gt, res, batches=batch)
    assert np.array_equal(got["precision"], one["precision"]) and np.array_equal(got["recall"], one["recall"])
    assert np.array_equal(got["stats"], one["stats"])
    _same(got, ref)


def test_deterministic(E, sets):
    gt, res, _ = sets[500]
    a, b = _device(E, gt, res), _device(E, gt, res)
    for k in ("precision", "recall", "stats"):
        assert np.array_equal(a[k], b[k]), k


def test_cell_beyond_lds_capacity(E):
    # 700 GTs in one (image, category) cell (the kernel keeps 256 in LDS; the rest of the code runs on global memory), 150 detections:
    # some exact, some near, many ties of IoU and score; plus a small cell in another image through the LDS path
    rng = np.random.default_rng(7)
    gts = [(float(20 * (j % 90)), float(20 * (j // 90)), 18 + (j % 3), 18 + (j % 5), 1) for j in range(700)]
    res = []
    for j in range(150):
        x, y, w, h, _ = gts[int(rng.integers(0, 700))]
        dx = float(rng.choice([0.0, 1.0, 3.0]))
        res.append(det(1, 1, (x + dx, y, w, h), np.floor(rng.uniform() * 16) / 16))
    gt = dataset({1: gts, 2: [(0, 0, 50, 50, 1), (10, 10, 50, 50, 1)]})
    res += [det(2, 1, (5, 5, 50, 50), .5), det(2, 1, (0, 0, 50, 50), .5)]
    got = _device(E, gt, res)
    ref = coco_eval_ref(gt, res)
    _same(got, ref)
    assert ref["recall"][0, 0, 0, 2] > 0.1


def test_no_detection_is_none(E):
    gt, _ = CASES["perfect"][0]()
    ev = E.CocoBoxEvaluator(gt, device="cuda:0")
    assert ev.compute() is None and ev.summary() == []
    ev.update([{"rois": np.zeros((0, 4), np.float32), "class_ids": np.zeros(0), "scores": np.zeros(0, np.float32)}], 1)
    assert ev.compute() is None


def test_eval_entry_point(E, sets, tmp_path, capsys):
    import json
    gt, res, ref = sets[37]
    p = tmp_path / "val_bbox_results.json"
    p.write_text(json.dumps(res))
    ids = [im["id"] for im in gt["images"]][:20]
    stats = E._eval(gt, ids, str(p))
    out = capsys.readouterr().out
    assert "Average Precision  (AP) @[ IoU=0.50:0.95 | area=   all | maxDets=100 ]" in out
    assert np.allclose(stats, coco_eval_ref(gt, res, img_ids=ids)["stats"], rtol=0, atol=1e-12)
