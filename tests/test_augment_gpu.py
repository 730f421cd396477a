"""Device augmentation (hn_augment.hip via augment.augment_batch) against the float64 numpy restatement (tests/augment_ref.py), batching,
label consistency and the trainer end to end on raw batches."""
import copy
import os

import numpy as np
import pytest
import torch
import yaml

import augment_ref as R
from multitask_hydranet_amd import augment as A

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _frame(rng, h, w):
    # smooth structure + noise: blur / warp / area all see real gradients
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([(xx * 255 // w), (yy * 255 // h), ((xx + yy) * 7) % 256], -1)
    return np.clip(base + rng.integers(-40, 41, (h, w, 3)), 0, 255).astype(np.uint8)


def _check_image(frame, plan, out_hw, got_chw):
    d = A.describe(plan, frame.shape[1], frame.shape[0])
    rgb, _ = R.image(frame, d, *out_hw)
    got = R.denormalize(got_chw)
    diff = np.abs(got - rgb.astype(np.int64))
    assert diff.max() <= 1, (plan, diff.max())
    assert (diff == 0).mean() >= 0.999, (plan, (diff == 0).mean())


def _check_seg(label, plan, out_hw, got):
    d = A.describe(plan, label.shape[1], label.shape[0])
    ref, alts, flag = R.seg(label, d["finv"], *out_hw)
    ok = (got == ref) | (flag & np.any([got == a for a in alts], axis=0))
    assert ok.all(), (plan, (~ok).sum())


PHOTO = [{"op": "blur", "sigma": 0.7}, {"op": "blur", "sigma": 1.5}, {"op": "contrast", "alpha": 1.5},
         {"op": "multiply", "per_channel": True, "factor": [0.8, 1.1, 1.2]}, {"op": "multiply", "per_channel": False, "factor": [1.13] * 3},
         {"op": "noise", "per_channel": True, "scale": 20.0}, {"op": "noise", "per_channel": False, "scale": 7.5},
         {"op": "hue", "factor": 1.27}, {"op": "sat", "factor": 1.9}, {"op": "val", "factor": 0.6}]
GEOM = [("fliplr", None), ("flipud", None), ("translate_x", -13), ("shear_x", 11.5), ("rotate", -14.2), ("crop", (0.2, 0.15, 0.0, 0.15))]


@pytest.mark.parametrize("src_hw,out_hw", [((1080, 1920), (640, 640)), ((1440, 2560), (512, 1024)), ((660, 1570), (128, 128)),
                                           ((721, 1283), (640, 640))])
def test_ops_against_reference(src_hw, out_hw):
    rng = np.random.default_rng(src_hw[0])
    frame = _frame(rng, *src_hw)
    label = (rng.integers(0, 4, (src_hw[0] // 8 + 1, src_hw[1] // 8 + 1)).repeat(8, 0).repeat(8, 1)[:src_hw[0], :src_hw[1]]).astype(np.uint8)
    plans = [dict(A.identity_plan(), augmented=True, photo=p, seed=1234567 + i) for i, p in enumerate(PHOTO)]
    plans += [dict(A.identity_plan(), augmented=True, geom=[g]) for g in GEOM]
    plans += [A.sample_plan(3, 0, i, do_flip=True) for i in range(6)]
    for i in range(0, len(plans), 8):
        chunk = plans[i:i + 8]
        out = A.augment_batch([frame] * len(chunk), None, None, [label] * len(chunk), chunk, out_hw, DEV)
        img, seg = out["image"].cpu().numpy(), out["gt_seg"].cpu().numpy()
        for j, p in enumerate(chunk):
            _check_image(frame, p, out_hw, img[j])
            _check_seg(label, p, out_hw, seg[j])


def test_identity_same_size_exact():
    rng = np.random.default_rng(1)
    frames = [_frame(rng, 128, 160), _frame(rng, 128, 160)]
    out = A.augment_batch(frames, None, None, None, [A.identity_plan()] * 2, (128, 160), DEV)
    ref = np.stack([R.normalize(f[..., ::-1]) for f in frames])
    assert np.array_equal(out["image"].cpu().numpy(), ref)


def test_ragged_batch_equals_single_and_repeats():
    rng = np.random.default_rng(2)
    frames = [_frame(rng, 1080, 1920), _frame(rng, 721, 1283), _frame(rng, 660, 1570)]
    segs = [rng.integers(0, 5, f.shape[:2]).astype(np.uint8) for f in frames]
    plans = [A.sample_plan(0, 0, i) for i in (1, 2, 3)]
    plans[0]["photo"] = {"op": "noise", "per_channel": True, "scale": 12.0}
    a = A.augment_batch(frames, None, None, segs, plans, (512, 640), DEV)
    b = A.augment_batch(frames, None, None, segs, plans, (512, 640), DEV)
    assert torch.equal(a["image"], b["image"]) and torch.equal(a["gt_seg"], b["gt_seg"])
    for i in range(3):
        s = A.augment_batch([frames[i]], None, None, [segs[i]], [plans[i]], (512, 640), DEV)
        assert torch.equal(s["image"][0], a["image"][i]) and torch.equal(s["gt_seg"][0], a["gt_seg"][i])


def test_labels_consistent_with_pixels():
    rng = np.random.default_rng(4)
    H, W = 720, 1280
    rects = [(100, 150, 300, 330), (700, 80, 900, 260), (500, 400, 760, 640)]
    frame = np.zeros((H, W, 3), np.uint8)
    seg = np.zeros((H, W), np.uint8)
    for k, (x1, y1, x2, y2) in enumerate(rects):
        frame[y1:y2, x1:x2] = 255
        seg[y1:y2, x1:x2] = k + 1
    boxes = np.array([[x1, y1, x2, y2, k] for k, (x1, y1, x2, y2) in enumerate(rects)], dtype=np.float64)
    plans = [A.sample_plan(21, 0, i) for i in range(40)]
    plans = [p for p in plans if p["geom"]][:8]
    out = A.augment_batch([frame] * len(plans), None, [boxes] * len(plans), [seg] * len(plans), plans, (H, W), DEV)
    img = out["image"].cpu().numpy()
    gseg = out["gt_seg"].cpu().numpy()
    det = out["gt_det"].cpu().numpy()
    for j in range(len(plans)):
        bright = R.denormalize(img[j])[..., 0] > 127
        assert ((gseg[j] > 0) == bright).mean() > 0.995           # the warped image and the label map agree
        for row in det[j]:
            if row[0] < 0:
                continue
            k = int(row[4])
            ys, xs = np.nonzero(gseg[j] == k + 1)
            if len(xs) == 0:
                continue
            assert xs.min() >= row[0] - 1 and xs.max() + 1 <= row[2] + 1 and ys.min() >= row[1] - 1 and ys.max() + 1 <= row[3] + 1


def _tiny_cfgs():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    return yaml.safe_load(open(os.path.join(root, "cfgs", "hydranet_tiny.yml")))


def _raw_batch(cfgs, rng, n, plans, same_size=True):
    from multitask_hydranet_amd.augment import pack
    h, w = cfgs["dataloader"]["network_input_height"], cfgs["dataloader"]["network_input_width"]
    sh = (h, w) if same_size else (h * 2 + 6, w * 2 + 10)
    frames = [_frame(rng, *sh) for _ in range(n)]
    segs = [rng.integers(0, len(cfgs["segment"]["class_list"]), sh).astype(np.uint8) for _ in range(n)]
    dets = [np.array([[10, 12, 60, 50, 0], [30, 5, 90, 40, 1]], dtype=np.float64) for _ in range(n)]
    lanes = [{"Lines": [[{"x": 20.0 + 3 * i, "y": float(sh[0] - 1)}, {"x": 40.0, "y": sh[0] / 2.0}, {"x": 60.0, "y": 5.0}]], "Labels": ["l"]}
             for i in range(n)]
    return dict(src_frames=pack(frames), src_segs=pack(segs), det_raw=dets, lane_raw=lanes, aug_plans=plans,
                src_image_shape=[dict(width=sh[1], height=sh[0], channel=3)] * n), frames, segs, dets, lanes


def _trainer(cfgs, capture):
    from multitask_hydranet_amd.train import HydraTrainer
    torch.manual_seed(0)
    tr = HydraTrainer(cfgs, iters_per_epoch=10, capture_step=capture)
    tr.hydranet.lane_points_per_line = int(cfgs["dataloader"]["network_input_height"] / cfgs["lane"]["interval"])   # the codec's P
    return tr


@pytest.mark.parametrize("capture", [False, True])
def test_trainer_identity_raw_equals_prepared(capture):
    import json
    cfgs = _tiny_cfgs()
    rng = np.random.default_rng(5)
    n = 2
    raw, frames, segs, dets, lanes = _raw_batch(cfgs, rng, n, [A.identity_plan()] * n)
    prepared = dict(image=torch.from_numpy(np.stack([R.normalize(f[..., ::-1]) for f in frames])),
                    gt_seg=torch.from_numpy(np.stack(segs)), gt_det=torch.from_numpy(A.pad_boxes(dets, [(1.0, 1.0)] * n)),
                    annot_lane=[json.dumps(l) for l in lanes], src_image_shape=raw["src_image_shape"])
    losses = []
    for b in (raw, prepared):
        tr = _trainer(cfgs, capture)
        seq = []
        for _ in range(4 if capture else 1):
            seq.append({k: float(v) for k, v in tr.train_step(copy.copy(b)).items()})
        losses.append(seq)
        del tr
    assert losses[0] == losses[1]


def test_trainer_random_plans_and_valid():
    cfgs = _tiny_cfgs()
    rng = np.random.default_rng(6)
    tr = _trainer(cfgs, False)
    for step in range(3):
        raw = _raw_batch(cfgs, rng, 2, [A.sample_plan(1, step, i) for i in range(2)], same_size=False)[0]
        ld = tr.train_step(raw)
        assert all(np.isfinite(float(v)) for v in ld.values())
    tr.validloader = [_raw_batch(cfgs, rng, 2, [A.identity_plan()] * 2, same_size=False)[0]]
    tr.valid(0)
    assert len(tr.last_valid["losses"]) == 1 and np.isfinite(tr.last_valid["losses"][0]["total_loss"])
