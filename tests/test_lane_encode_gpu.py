"""GPU: lane ground-truth encoding on the device (hn_lane_encode via LaneCodec.encode_lanes / encode_lane, and HydraTrainer.to_gpu for
batches that carry only the raw annotations) held to the reference's recorded outputs (tests/golden/lane_encode_kats.npz) and to the fp64
restatement (tests/lane_encode_ref.py) on random batches."""
import json

import numpy as np
import pytest
import torch

from tests.helpers import load_cfg, load_npz, tiny_state
from tests.lane_encode_ref import encode_ref, parse_lanes

pytestmark = pytest.mark.gpu

GEOMS = ("g640i", "g640n", "g512x1024", "g128")


@pytest.fixture(scope="module")
def kats():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    import __graft_entry__ as g
    g.build()
    return load_npz("lane_encode_kats.npz")


def _codec(z, g):
    from multitask_hydranet_amd.lane_codec import LaneCodec
    W, H, S, P, ip, si, iv = (int(v) for v in z[g + "/meta"])
    return LaneCodec(W, H, S, P, do_interpolate=bool(ip), anchor_lane_num=1, scale_invariance=bool(si)), P, iv


def _inputs(z, g):
    return [str(a) for a in z[g + "/annot"]], [tuple(int(v) for v in s) for s in z[g + "/src"]]


@pytest.mark.parametrize("g", GEOMS)
def test_every_fixture_image(kats, g):
    codec, P, iv = _codec(kats, g)
    objs, srcs = _inputs(kats, g)
    differ = 0
    for k in range(len(objs)):
        cls, loc = codec.encode_lanes([objs[k]], [srcs[k]], div_interval=iv)
        cls, loc = cls[0].cpu().numpy(), loc[0].cpu().numpy()
        ec, el = kats[g + "/gt_cls"][k], kats[g + "/gt_loc"][k]
        assert np.array_equal(cls, ec), (g, k, np.argwhere(cls != ec)[:5])
        assert np.array_equal(loc[:, P:P + 2], el[:, P:P + 2]), (g, k)
        assert np.abs(loc - el).max() <= 1e-4, (g, k, np.abs(loc - el).max())
        differ += int((loc != el).sum())
    print("%s: %d gt_loc entries not bitwise equal to the reference" % (g, differ))


@pytest.mark.parametrize("g", GEOMS)
def test_batch_equals_per_image_permutes_and_repeats(kats, g):
    codec, P, iv = _codec(kats, g)
    objs, srcs = _inputs(kats, g)
    cls, loc = codec.encode_lanes(objs, srcs, div_interval=iv)
    for k in range(len(objs)):
        c1, l1 = codec.encode_lanes([objs[k]], [srcs[k]], div_interval=iv)
        assert torch.equal(cls[k], c1[0]) and torch.equal(loc[k], l1[0]), (g, k)
    perm = np.random.default_rng(5).permutation(len(objs))
    cp, lp = codec.encode_lanes([objs[i] for i in perm], [srcs[i] for i in perm], div_interval=iv)
    assert torch.equal(cp, cls[perm]) and torch.equal(lp, loc[perm])
    c2, l2 = codec.encode_lanes(objs, srcs, div_interval=iv)
    assert torch.equal(c2, cls) and torch.equal(l2, loc)


def _random_batch(rng, n, ow, oh):
    objs = []
    for _ in range(n):
        lines = []
        for _ in range(int(rng.integers(0, 9))):
            m = int(rng.integers(1, 301))
            x0, x1 = rng.uniform(-0.15, 1.15) * ow, rng.uniform(0.2, 0.8) * ow
            y0, y1 = rng.uniform(0.7, 1.1) * oh, rng.uniform(0.25, 0.65) * oh
            t = np.sort(rng.uniform(0, 1, m))
            xs = x0 + (x1 - x0) * t + rng.uniform(-0.06, 0.06) * ow * t * (1 - t) * 4
            ys = y0 + (y1 - y0) * t
            pts = [{"x": float(x), "y": float(y)} for x, y in zip(xs, ys)]
            lines.append(pts if rng.integers(2) else pts[::-1])
        objs.append({"Lines": lines})
    return objs


@pytest.mark.parametrize("W,H,interp", [(640, 640, True), (640, 640, False), (1024, 512, True)])
def test_random_batches_against_restatement(kats, W, H, interp):
    from multitask_hydranet_amd.lane_codec import LaneCodec
    P = H // 8
    codec = LaneCodec(W, H, 32, P, do_interpolate=interp, anchor_lane_num=1, scale_invariance=True)
    rng = np.random.default_rng(W + H + int(interp))
    objs = _random_batch(rng, 16, 2560, 1440)
    cls, loc = codec.encode_lanes(objs, [(2560, 1440)] * 16, div_interval=8)
    cls, loc = cls.cpu().numpy(), loc.cpu().numpy()
    differ = 0
    for k, o in enumerate(objs):
        ec, el = encode_ref(parse_lanes(o, W, H, 2560, 1440), W, H, 32, P, interp, True, 8)
        assert np.array_equal(cls[k], ec), k
        assert np.array_equal(loc[k][:, P:P + 2], el[:, P:P + 2]), k
        assert np.abs(loc[k] - el).max() <= 1e-4, k
        differ += int((loc[k] != el).sum())
    assert (cls[:, :, 1] == 1).sum() > 100
    print("%dx%d interpolate=%s: %d gt_loc entries not bitwise equal to the restatement" % (W, H, interp, differ))


def test_encode_lane_returns_reference_types(kats):
    from multitask_hydranet_amd.lane_codec import LaneCodec
    g = "g512x1024"                                   # scale_invariance off: the recorded rows are encode_lane's own
    codec, P, iv = _codec(kats, g)
    objs, srcs = _inputs(kats, g)
    for k in range(len(objs)):
        gt_type, gt_loc = codec.encode_lane(json.loads(objs[k]), srcs[k][0], srcs[k][1])
        assert isinstance(gt_type, np.ndarray) and isinstance(gt_loc, np.ndarray)
        assert gt_type.dtype == np.float32 and gt_loc.dtype == np.float32
        assert gt_type.shape == (codec.feature_size, 2) and gt_loc.shape == (codec.feature_size, 2 * P + 2)
        assert np.array_equal(gt_type, kats[g + "/gt_cls"][k]) and np.abs(gt_loc - kats[g + "/gt_loc"][k]).max() <= 1e-4
    # encode_lane returns the rows BEFORE the division even with scale_invariance
    c2, P2, iv2 = _codec(kats, "g640i")
    o2, s2 = _inputs(kats, "g640i")
    _, raw = c2.encode_lane(o2[-1], *s2[-1])
    want = kats["g640i/gt_loc"][len(o2) - 1]
    assert np.abs(raw[:, :P2] / np.float32(8) - want[:, :P2]).max() <= 1e-4
    two = LaneCodec(640, 640, 32, 80, do_interpolate=True, anchor_lane_num=2)
    assert two.encode_lane(json.loads(objs[0]), *srcs[0]) == (None, None)


def test_trainer_encodes_missing_lane_targets(kats):
    """the tiny fixture batch with its lane targets replaced by the 128x128 fixtures: carrying gt_loc / gt_cls, or only annot_lane +
    src_image_shape, gives bitwise-equal losses, eager and with the captured step"""
    from multitask_hydranet_amd.train import HydraTrainer
    z = load_npz("tiny_hydranet.npz")
    cfgs = load_cfg("hydranet_tiny.yml")
    cfgs["train"].update(dict(continue_train=False, weight_file="", epoch=1, lr=1e-4, weight_decay=0.0))
    batch = {k[3:]: torch.from_numpy(z[k].copy()) for k in z.files if k.startswith("in/")}
    n = batch["image"].shape[0]
    assert cfgs["lane"]["interpolate"] and cfgs["lane"]["scale_invariance"]
    with_gt = dict(batch, gt_cls=torch.from_numpy(kats["g128/gt_cls"][:n].copy()), gt_loc=torch.from_numpy(kats["g128/gt_loc"][:n].copy()))
    raw = {k: v for k, v in batch.items() if k not in ("gt_cls", "gt_loc")}
    raw["annot_lane"] = np.stack([str(a) for a in kats["g128/annot"][:n]])
    raw["src_image_shape"] = np.stack([dict(width=int(s[0]), height=int(s[1]), channel=3) for s in kats["g128/src"][:n]])
    gen = torch.Generator().manual_seed(7)
    noise = [0.05 * torch.randn(batch["image"].shape, generator=gen) for _ in range(4)]
    for capture in (False, True):
        runs = []
        for src in (with_gt, raw):
            tr = HydraTrainer(cfgs, trainloader=None, validloader=None, iters_per_epoch=4, capture_step=capture)
            tr.hydranet.load_state_dict(tiny_state(z))
            tr.hydranet.lane_points_per_line = int(z["meta/lane_points_per_line"])
            losses = []
            for it in range(4):
                b = {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in src.items()}
                b["image"] = batch["image"] + noise[it]
                ld = tr.train_step(b)
                losses.append({k: float(v.detach()) for k, v in ld.items()})
            assert (tr._cap is not None) == capture
            runs.append(losses)
        assert all(l["loss_lane_loc"] > 0 for l in runs[0])
        for step, (a, b) in enumerate(zip(*runs)):
            assert a == b, (capture, step, a, b)
