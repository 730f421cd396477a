"""GPU: the lane F1 of a whole batch on the device (lane_metric.LaneIoUBatch / iou_matrices / LaneMetric(batched=True),
hn_lane_metric.hip) against the recording the reference's own lane_metric.py made of one ragged batch
(tests/golden/lane_metric_batch.json), against the oracle's numpy rasteriser, and against the per-image path (iou_matrix,
LaneMetric(batched=False)).  Everything is integer counts and float64 ratios of them: sample points and count tables are compared for
equality, IoU matrices at 1e-12.  SELF-CONSISTENCY ONLY for the thick-line fill rule, as in test_post_gpu.py's
test_lane_metric_device_vs_reference_recording: cv2 is absent, the recording was made with the oracle's cv2_line stand-in."""
import copy
import json
import os

import numpy as np
import pytest
import torch

from tests.helpers import load_cfg, load_npz, tiny_state

pytestmark = pytest.mark.gpu
WIDTHS = (30, 10)
THRESH_LISTS = ([0.5], [0.3, 0.5, 0.7])
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def pkg():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    import __graft_entry__ as g
    g.build()
    import multitask_hydranet_amd as P
    from oracle import hydranet_oracle as O
    return P, O


@pytest.fixture(scope="module")
def rec():
    return json.load(open(os.path.join(GOLDEN, "lane_metric_batch.json")))


def eval_lanes(pair):
    gts = [ln for ln in pair["gt_result"]["Lines"] if len(ln) > 0]
    prs = [ln["points"] if "score" in ln else ln for ln in pair["pr_result"]["Lines"]]
    return gts, [ln for ln in prs if len(ln) > 0]


def items_of(images):
    return [(*eval_lanes(p), p["gt_result"]["Shape"]["height"], p["gt_result"]["Shape"]["width"]) for p in images]


def test_fixture_batch_samples_iou_and_counts(pkg, rec):
    """(1) one launch sequence for the 12 images of three frame sizes: the int-truncated spline samples the device painted from == the
    reference's (integer equality: float64 spline without FMA contraction), every IoU matrix == calc_iou's at 1e-12, and the count tables
    == those of the per-image path (hn_lane_raster + hn_lane_iou through full-frame masks)"""
    from multitask_hydranet_amd import lane_metric as LM
    items = items_of(rec["images"])
    for lw in WIDTHS:
        b = LM.LaneIoUBatch(lw, keep_samples=True)
        assert [b.add(*it) for it in items] == list(range(len(items)))
        res = b.result()
        mats = LM.iou_matrices(items, lw)
        assert len(res) == len(mats) == len(items)
        smp = b.samples()
        for k, (gts, prs, h, w) in enumerate(items):
            want = [np.stack([np.cumsum(l["dx"]), np.cumsum(l["dy"])], axis=1).reshape(-1, 2) for l in rec["samples"][k]]
            assert len(smp[k]) == len(want) == len(gts) + len(prs)
            for got, wnt in zip(smp[k], want):
                assert got.dtype == np.int32 and np.array_equal(got, wnt), (lw, k)
            r = res[k]
            assert r["iou"].shape == (len(gts), len(prs)) and r["iou"].dtype == np.float64 and r["inter"].shape == (len(gts), len(prs))
            assert np.array_equal(mats[k], r["iou"])
            np.testing.assert_allclose(r["iou"], np.array(rec["iou"][str(lw)][k], dtype=np.float64).reshape(r["iou"].shape), rtol=0, atol=1e-12,
                                       err_msg=f"{lw} {k}")
            if gts and prs:
                np.testing.assert_array_equal(r["iou"], LM.iou_matrix(gts, prs, h, w, lw))
                # the per-image path's integer tables, through its two kernels
                union = r["area_gt"][:, None] + r["area_pr"][None, :] - r["inter"]
                assert (r["inter"] <= np.minimum(r["area_gt"][:, None], r["area_pr"][None, :])).all() and (union >= 0).all()
                inter, area = _per_image_counts(LM, gts, prs, h, w, lw)
                assert np.array_equal(r["inter"], inter) and np.array_equal(np.concatenate([r["area_gt"], r["area_pr"]]), area), (lw, k)
        assert max(r["iou"].max() for r in res if r["iou"].size) > 0.5                            # (the recording has hits at both widths)
        assert res[3]["iou"].shape == (2, 0) and res[4]["iou"].shape == (0, 2) and res[5]["iou"].shape == (0, 0)
        assert (res[3]["area_gt"] > 0).all() and (res[4]["area_pr"] > 0).all()                    # a lane's area without a partner


def _per_image_counts(LM, gts, prs, h, w, lw):
    """|g & p| and the areas as iou_matrix computes them (hn_lane_raster into masks, hn_lane_iou)"""
    from multitask_hydranet_amd._lib import lib
    dev = torch.device("cuda", torch.cuda.current_device())
    pts, seg_lane, seg_first = [], [], []
    for li, lane in enumerate(list(gts) + list(prs)):
        ip = LM.spline_interp(lane=lane, step_t=1)
        base = len(pts)
        pts += [(int(q["x"]), int(q["y"])) for q in ip]
        for i in range(len(ip) - 1):
            seg_lane.append(li)
            seg_first.append(base + i)
    g, p = len(gts), len(prs)
    assert g <= 32 and p <= 32
    masks = torch.zeros((g + p, h, w), dtype=torch.uint8, device=dev)
    if seg_lane:
        tp = torch.tensor(pts, dtype=torch.int32).to(dev)
        tl, tf = torch.tensor(seg_lane, dtype=torch.int32).to(dev), torch.tensor(seg_first, dtype=torch.int32).to(dev)
        lib().call("hn_lane_raster", tp.data_ptr(), tl.data_ptr(), tf.data_ptr(), len(seg_lane), int(lw), h, w, masks.data_ptr())
    inter = torch.zeros((g, p), dtype=torch.int64, device=dev)
    area = torch.zeros((g + p,), dtype=torch.int64, device=dev)
    lib().call("hn_lane_iou", masks.data_ptr(), g, p, h * w, inter.data_ptr(), area.data_ptr())
    return inter.cpu().numpy(), area.cpu().numpy()


def _run_metric(LM, images, lw, tl, batched, chunks=None):
    m = LM.LaneMetric(method="f1_measure", iou_thresh=0.5, lane_width=lw, thresh_list=tl, batched=batched)
    m.reset()
    for c in (chunks or [images]):
        m(output=c)
    return m


def test_batched_metric_equals_recording_and_per_image_path(pkg, rec):
    """(2) LaneMetric(batched=True): result_record and summary() of every handler and the metric's summary() == the reference's recording
    and == LaneMetric(batched=False), for both lane widths and both thresh_lists, on the batch fixture and on the four images of
    lane_metric.json; two calls (images 0-5, then 6-11) give the records of one call; reset() empties them"""
    from multitask_hydranet_amd import lane_metric as LM
    imgs = rec["images"]
    old = json.load(open(os.path.join(GOLDEN, "lane_metric.json")))
    for lw in WIDTHS:
        for tl in THRESH_LISTS:
            want = rec["results"]["%d|%s" % (lw, ",".join("%g" % t for t in tl))]
            m = _run_metric(LM, imgs, lw, tl, True)
            ref = _run_metric(LM, imgs, lw, tl, False)
            two = _run_metric(LM, imgs, lw, tl, True, chunks=[imgs[:6], imgs[6:]])
            assert len(m.metric_handlers) == len(tl)
            for h, hr, h2, hw in zip(m.metric_handlers, ref.metric_handlers, two.metric_handlers, want["handlers"]):
                assert h.result_record == hw["records"] and h.summary() == hw["summary"], (lw, tl, h.prob_thresh)
                assert h.result_record == hr.result_record and h.summary() == hr.summary()
                assert h2.result_record == hw["records"] and h2.summary() == hw["summary"]
            assert m.summary() == want["summary"] == ref.summary() == two.summary()
            m.reset()
            assert all(h.result_record == [] for h in m.metric_handlers)
            m(output=imgs[:2])
            assert [h.result_record for h in m.metric_handlers] == [hw["records"][:2] for hw in want["handlers"]]
        for thr in (0.5, 0.3):
            want = old["results"]["%d,%g" % (lw, thr)]
            m = _run_metric(LM, old["images"], lw, [thr], True)
            ref = _run_metric(LM, old["images"], lw, [thr], False)
            h = m.metric_handlers[0]
            assert h.result_record == want["records"] == ref.metric_handlers[0].result_record
            assert h.summary() == want["summary"] == ref.metric_handlers[0].summary() and m.summary() == want["f1"] == ref.summary()
    m = LM.LaneMetric(method="recall", iou_thresh=0.5, lane_width=30, batched=True)              # no thresh_list: one handler, no score test
    m(output=[p for p in imgs if not any("score" in ln for ln in p["pr_result"]["Lines"])])
    ref = LM.LaneMetric(method="recall", iou_thresh=0.5, lane_width=30)
    ref(output=[p for p in imgs if not any("score" in ln for ln in p["pr_result"]["Lines"])])
    assert m.metric_handlers[0].result_record == ref.metric_handlers[0].result_record and m.summary() == ref.summary()


def test_full_frame_image_batched_with_a_small_one(pkg):
    """(3) one 1080 x 1920 image (510 tiles) with 3 x 3 lanes of 11 points, in one batch with a 96 x 160 image: every pair == the oracle's
    numpy rasteriser"""
    P, O = pkg
    from multitask_hydranet_amd import lane_metric as LM
    rs = np.random.RandomState(2)
    gts = [[{"x": float(200 + 300 * j + 15 * i + 0.8 * i * i * (j - 2)), "y": float(1070 - 90 * i)} for i in range(11)] for j in range(3)]
    prs = [[{"x": p["x"] + float(rs.randint(-20, 20)), "y": p["y"]} for p in g] for g in gts]
    sg = [[{"x": 20.0 + 4 * i, "y": 90.0 - 20 * i} for i in range(5)], [{"x": 120.0, "y": 95.0}, {"x": 90.0, "y": 5.0}]]
    sp = [[{"x": 24.0 + 4 * i, "y": 90.0 - 20 * i} for i in range(5)]]
    big, small = LM.iou_matrices([(gts, prs, 1080, 1920), (sg, sp, 96, 160)], 30)
    ref = np.array([[O.lane_iou(g, p, 1080, 1920, 30) for p in prs] for g in gts])
    np.testing.assert_allclose(big, ref, rtol=0, atol=1e-12)
    assert big.shape == (3, 3) and big.max() > 0.5
    np.testing.assert_allclose(small, np.array([[O.lane_iou(g, p, 96, 160, 30) for p in sp] for g in sg]), rtol=0, atol=1e-12)


def test_more_than_one_pair_block(pkg):
    """(4) 37 ground truths x 41 predictions at 512 x 2048 (2 x 2 blocks of 32 x 32 pairs) in a batch with a 3 x 2 image == the per-image
    path's matrix, exactly"""
    from multitask_hydranet_amd import lane_metric as LM
    many_g = [[{"x": float(40 + 45 * j + 3 * i), "y": float(500 - 40 * i)} for i in range(8)] for j in range(37)]
    many_p = [[{"x": float(30 + 42 * j + 4 * i), "y": float(500 - 40 * i)} for i in range(8)] for j in range(41)]
    sg = [[{"x": 30.0 + 50 * j + 2 * i, "y": 120.0 - 25 * i} for i in range(5)] for j in range(3)]
    sp = [[{"x": 33.0 + 50 * j + 2 * i, "y": 120.0 - 25 * i} for i in range(5)] for j in range(2)]
    small, big = LM.iou_matrices([(sg, sp, 128, 200), (many_g, many_p, 512, 2048)], 30)
    assert big.shape == (37, 41) and small.shape == (3, 2)
    np.testing.assert_array_equal(big, LM.iou_matrix(many_g, many_p, 512, 2048, 30))
    np.testing.assert_array_equal(small, LM.iou_matrix(sg, sp, 128, 200, 30))
    assert big.max() > 0.3 and small.max() > 0.5


def test_trainer_valid_lane_f1(pkg):
    """(5) HydraTrainer.valid over two batches that carry gt_lane_json (the validation of test_train_gpu.py's
    test_valid_writes_coco_results_and_lane_json): last_valid["lane_f1"] == LaneMetric(batched=False) fed with last_valid["lane_result"] and
    the same ground truth.  The ground truth is made from a first run's predictions (kept, shifted, dropped), so there are hits and misses."""
    from multitask_hydranet_amd import lane_metric as LM
    from multitask_hydranet_amd.lane_codec import LaneCodec
    from multitask_hydranet_amd.train import HydraTrainer
    z = load_npz("tiny_hydranet.npz")
    cfgs = load_cfg("hydranet_tiny.yml")
    cfgs["train"].update(dict(continue_train=False, weight_file="", epoch=1, lr=1e-4, weight_decay=0.0))
    cfgs["lane"]["conf_thres"] = 0.3                                                             # scores on both sides of the metric's 0.5
    batch = {k[3:]: torch.from_numpy(z[k].copy()) for k in z.files if k.startswith("in/")}
    n = batch["image"].shape[0]
    shapes = [{"width": 1920, "height": 1080}] * n
    h, w = batch["image"].shape[2], batch["image"].shape[3]
    coder = LaneCodec(w, h, cfgs["lane"]["anchor_stride"], h // cfgs["lane"]["interval"])

    sd = tiny_state(z)

    def trainer(loader):
        tr = HydraTrainer(copy.deepcopy(cfgs), trainloader=[dict(batch)], validloader=loader, iters_per_epoch=1)
        tr.hydranet.load_state_dict(sd)
        tr.hydranet.lane_points_per_line = int(z["meta/lane_points_per_line"])
        return tr
    # the fixture's random lane head calls every anchor background and gives its lanes no points: shift the lane logit's bias so that a
    # fifth of the anchors score above one half, and the two point counts (the decode, the NMS and the metric then see lanes with scores on
    # both sides of the threshold)
    tr = trainer([])
    net = tr.hydranet.eval()
    with torch.no_grad():
        logits = net(batch["image"].to(tr.device).float())["lane"]["predict_cls"].float()
    margin = (logits[..., 0] - logits[..., 1]).flatten()
    sd["laneheader.conv_cls_conv.3.bias"] = sd["laneheader.conv_cls_conv.3.bias"].clone()
    sd["laneheader.conv_cls_conv.3.bias"][1] += float(torch.quantile(margin, 0.8))
    ppl = int(z["meta/lane_points_per_line"])
    for name, k in (("laneheader.conv_down_conv.3.bias", ppl), ("laneheader.conv_up_conv.3.bias", 0)):
        sd[name] = sd[name].clone()
        sd[name][k] += 6.0                                                                        # six points below and above the anchor
    tr = trainer([dict(batch, src_image_shape=shapes)])
    tr.valid(0, lane_coder=coder)
    assert tr.last_valid["lane_f1"] is None                                                      # no ground truth, no metric
    first = [r["pr_result"]["Lines"] for r in tr.last_valid["lane_result"]]
    assert sum(len(l) for l in first) >= 2, "the tiny model predicts no lanes at this threshold"
    gts = []
    for i, lines in enumerate(first):
        g = []
        for j, ln in enumerate(lines):
            if (i + j) % 3 == 2:
                continue                                                                         # a false positive
            off = 3.0 if (i + j) % 3 == 0 else 40.0                                              # a hit / a miss
            g.append([{"x": p["x"] + off, "y": p["y"]} for p in ln["points"]])
        g.append([{"x": 100.0 + 30 * k, "y": 1000.0 - 80 * k} for k in range(6)])                # a lane nobody predicted
        gts.append({"Lines": g, "Labels": [1] * len(g)})
    tr = trainer([dict(batch, src_image_shape=shapes, gt_lane_json=gts), dict(batch, src_image_shape=shapes, gt_lane_json=gts[::-1])])
    tr.valid(0, lane_coder=coder)
    lv = tr.last_valid
    assert len(lv["lane_result"]) == 2 * n
    gt_all = gts + gts[::-1]
    pairs = [dict(pr_result=r["pr_result"], gt_result={**g, "Shape": r["pr_result"]["Shape"]}) for r, g in zip(lv["lane_result"], gt_all)]
    ref = LM.LaneMetric(method="f1_measure", iou_thresh=0.5, lane_width=30, thresh_list=[0.5])
    ref(output=pairs)
    assert lv["lane_f1"] == ref.summary()
    assert sum(r["gt_num"] for r in ref.metric_handlers[0].result_record) > 0
    print("lane_f1", lv["lane_f1"], ref.metric_handlers[0].result_record)
