"""GPU, end to end: HydraTrainer.valid(coco_gt=...) on the tiny cfg (the validation of tests/test_train_gpu.py's
test_valid_writes_coco_results_and_lane_json) evaluates its detections on the device: last_valid["det_eval"] equals det_eval._eval on
the val_bbox_results.json the same call wrote, and the fp64 restatement on those records; without coco_gt last_valid keeps its keys."""
import json

import numpy as np
import pytest
import torch

from tests.coco_eval_ref import coco_eval_ref
from tests.helpers import load_cfg, load_npz, tiny_state

pytestmark = pytest.mark.gpu
KEYS = {"losses", "detect_result", "detect_json", "lane_result", "iou", "lane_f1"}


@pytest.fixture(scope="module")
def setup():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    import __graft_entry__ as g
    g.build()
    z = load_npz("tiny_hydranet.npz")
    cfgs = load_cfg("hydranet_tiny.yml")
    cfgs["train"].update(dict(continue_train=False, weight_file="", epoch=1, lr=1e-4, weight_decay=0.0))
    batch = {k[3:]: torch.from_numpy(z[k].copy()) for k in z.files if k.startswith("in/")}
    return z, cfgs, batch


def _trainer(setup):
    from multitask_hydranet_amd.train import HydraTrainer
    z, cfgs, batch = setup
    vb = dict(batch)
    vb["src_image_shape"] = [{"width": 1920, "height": 1080}] * batch["image"].shape[0]
    tr = HydraTrainer(cfgs, trainloader=[dict(batch)], validloader=[vb, dict(vb)], iters_per_epoch=1)
    tr.hydranet.load_state_dict(tiny_state(z))
    tr.hydranet.lane_points_per_line = int(z["meta/lane_points_per_line"])
    return tr


def _ground_truth(setup):
    """gen_coco_label's dict from the batch's boxes at source scale (network input -> 1920 x 1080), one GT image per validation image"""
    from multitask_hydranet_amd.coco_json import coco_ground_truth
    z, cfgs, batch = setup
    n, h, w = batch["image"].shape[0], batch["image"].shape[2], batch["image"].shape[3]
    ann = batch["gt_det"].numpy()
    recs = []
    for rep in range(2):                               # the loader yields the batch twice: image ids 1..n, n+1..2n
        for i in range(n):
            rows = [r for r in ann[i] if r[4] >= 0]
            annos = [(r[0] * 1920 / w, r[1] * 1080 / h, r[2] * 1920 / w, r[3] * 1080 / h, int(r[4]) + 1) for r in rows]
            recs.append({"file_name": "img%d_%d.jpg" % (rep, i), "height": 1080, "width": 1920, "annos": annos})
    return coco_ground_truth(recs)


def test_valid_reports_coco_map(setup, tmp_path, capsys):
    from multitask_hydranet_amd.det_eval import _eval
    gt = _ground_truth(setup)
    assert len(gt["images"]) == 2 * setup[2]["image"].shape[0] and gt["annotations"]
    tr = _trainer(setup)
    tr.valid(0, eval_dir=str(tmp_path), det_conf_thres=0.02, coco_gt=gt)
    lv = tr.last_valid
    assert set(lv) == KEYS | {"det_eval"}
    out = capsys.readouterr().out
    assert "metric detection 0" in out and "Average Recall     (AR) @[ IoU=0.50:0.95 | area=   all | maxDets=100 ]" in out
    res = lv["det_eval"]
    assert res is not None and lv["detect_result"]
    records = json.load(open(lv["detect_json"]))
    stats = _eval(gt, [im["id"] for im in gt["images"]][:tr.cfgs["detection"]["max_images"]], lv["detect_json"])
    assert np.array_equal(res["stats"], stats)
    ref = coco_eval_ref(gt, records)
    assert np.array_equal(res["precision"], ref["precision"]) and np.array_equal(res["recall"], ref["recall"])
    assert np.allclose(res["stats"], ref["stats"], rtol=0, atol=1e-12)


def test_valid_without_coco_gt_keeps_keys(setup, tmp_path):
    tr = _trainer(setup)
    tr.valid(0, eval_dir=str(tmp_path), det_conf_thres=0.02)
    assert set(tr.last_valid) == KEYS
