"""CPU: the numpy reference of the detection NMS options (tests/det_nms_ref.py) is anchored to the pinned oracle's post-process, the
NmsOptions / cfg validation, and the conditions that keep the GPU comparisons (tests/test_det_nms_gpu.py) from passing vacuously."""
import numpy as np
import pytest
import torch

from multitask_hydranet_amd.model import _det_nms_options
from multitask_hydranet_amd.postprocess import NMS_KINDS, NmsOptions
from oracle import hydranet_oracle as O
from tests import det_nms_ref as R
from tests.helpers import load_npz

THR, IOU, SIGMA = 0.05, 0.5, 0.5


def _same_as_oracle(hw, anchors, reg, cls, thr, iou):
    """reference with the hard defaults == oracle.postprocess: kept classes, scores and boxes, bit for bit"""
    ref = O.postprocess(hw, torch.stack([torch.from_numpy(anchors)] * len(reg)), torch.from_numpy(reg), torch.from_numpy(cls), thr, iou)
    mine = R.nms_batch(anchors, reg, cls, hw, thr, iou)
    kept = 0
    for (_, c, b, s), r in zip(mine, ref):
        assert np.array_equal(c, np.asarray(r["class_ids"], np.int64))
        assert np.array_equal(s, np.asarray(r["scores"], np.float32))
        assert np.array_equal(b.reshape(-1, 4), np.asarray(r["rois"], np.float32).reshape(-1, 4))
        kept += len(c)
    return kept


def test_reference_hard_equals_oracle_on_the_recorded_deploy_tensors():
    z = load_npz("tiny_hydranet.npz")
    anc = z["out/anchors"]
    anc = anc[0] if anc.ndim == 3 else anc
    hw = tuple(z["in/image"].shape[2:])
    assert _same_as_oracle(hw, anc, z["deploy/regression"], z["deploy/classification"], float(z["deploy/pp_thresh"]), 0.3) > 0


@pytest.mark.parametrize("seed,iou", [(0, 0.3), (1, 0.5)])
def test_reference_hard_equals_oracle_on_random_inputs(seed, iou):
    """real-valued boxes (non-zero regression), clipped boxes, score ties, an image with nothing over the threshold"""
    g = np.random.default_rng(seed)
    a, n, k = 600, 3, 4
    cy, cx = g.uniform(0, 96, a), g.uniform(0, 160, a)
    hh, ww = g.uniform(4, 40, a), g.uniform(4, 40, a)
    anchors = np.stack([cy - hh, cx - ww, cy + hh, cx + ww], axis=1).astype(np.float32)
    reg = (g.standard_normal((n, a, 4)) * 0.2).astype(np.float32)
    cls = (g.uniform(0, 1, (n, a, k)) ** 4).astype(np.float32)
    cls[0, 100:110, 2] = 0.75
    cls[2] *= 0.01
    assert _same_as_oracle((96, 160), anchors, reg, cls, 0.3, iou) > 20


def test_nms_options_validation():
    assert NMS_KINDS == R.KINDS
    o = NmsOptions()
    assert (o.kind, o.sigma, o.score_floor, o.max_det, o.class_agnostic) == ("hard", 0.5, None, 0, False)
    o = NmsOptions("soft_gaussian", sigma=0.25, score_floor=0.01, max_det=100, class_agnostic=True)
    assert (o.kind, o.sigma, o.score_floor, o.max_det, o.class_agnostic) == ("soft_gaussian", 0.25, 0.01, 100, True)
    assert o == NmsOptions("soft_gaussian", 0.25, 0.01, 100, True) and o != NmsOptions()
    for bad in (dict(kind="matrix"), dict(kind=None), dict(sigma=0), dict(sigma=-1.0), dict(sigma=float("inf")), dict(sigma=float("nan")),
                dict(max_det=-1), dict(max_det=1.5)):
        with pytest.raises(ValueError):
            NmsOptions(**bad)


def test_cfg_keys_validation():
    assert _det_nms_options({"num_classes": 9}) is None
    assert _det_nms_options({"max_det": 100}) == NmsOptions(max_det=100)
    assert _det_nms_options({"nms_type": "soft_gaussian", "nms_sigma": 0.3, "nms_score_floor": 0.01, "nms_class_agnostic": True}) == \
        NmsOptions("soft_gaussian", 0.3, 0.01, 0, True)
    for bad in ({"nms_type": "soft"}, {"nms_sigma": 0}, {"nms_sigma": "x"}, {"max_det": -3}, {"max_det": True}, {"nms_class_agnostic": 1},
                {"nms_score_floor": "low"}):
        with pytest.raises(ValueError, match="detection\\."):
            _det_nms_options(bad)


@pytest.fixture(scope="module")
def base():
    anchors, reg, cls = R.recipe()
    run = lambda **kw: R.nms_image(anchors, reg, cls, (128, 128), THR, IOU, sigma=SIGMA, **kw)
    return {(k, ag): run(kind=k, class_agnostic=ag) for k in R.KINDS for ag in (False, True)}, run, cls


def test_conditions_on_the_base_recipe(base):
    """what makes the recipe discriminate between the rules (asserted on the reference alone)"""
    res, run, cls = base
    n_over = int(R.count_over(cls[None], THR)[0])
    raw = cls.max(axis=1)
    hard = res["hard", False]
    assert n_over > 200 and len(np.unique(raw[raw > THR])) < n_over                        # equal scores occur
    assert set(res["diou", False][0]) != set(hard[0])                                       # diou keeps another set
    for k in ("soft_linear", "soft_gaussian"):
        idx, _, _, s = res[k, False]
        assert len(idx) > len(hard[0])                                                      # soft kinds keep more
        assert int((s != raw[idx]).sum()) >= 10                                             # ... with decayed scores
        assert np.all(s[1:] <= s[:-1]) and np.all(s > np.float32(THR))                      # descending, above the floor
    for k in R.KINDS:
        a, b = res[k, False], res[k, True]
        assert len(a[0]) != len(b[0]) or not np.array_equal(a[0], b[0]) or not np.array_equal(a[3], b[3]), k
    for k in ("hard", "soft_gaussian"):
        full, cut = res[k, False], run(kind=k, max_det=10)
        assert len(full[0]) > 10 and len(cut[0]) == 10                                      # max_det = 10 truncates
        for u, v in zip(full, cut):
            assert np.array_equal(u[:10], v)                                                # ... to the unlimited output's prefix
    assert np.array_equal(hard[3], raw[hard[0]])                                            # hard NMS returns raw scores


def test_reference_edge_cases():
    """no candidate, one candidate, zero-area boxes (NaN IoU suppresses and decays nothing), score_floor"""
    an = np.array([[5, 5, 5, 5]] * 4 + [[0, 0, 127, 127]], np.float32)
    reg = np.zeros((5, 4), np.float32)
    cls = np.array([[0.5], [0.5], [0.25], [0.75], [0.625]], np.float32)
    for k in R.KINDS:
        idx, _, _, s = R.nms_image(an, reg, cls, (128, 128), THR, IOU, kind=k)
        assert list(idx) == [3, 4, 0, 1, 2] and list(s) == [0.75, 0.625, 0.5, 0.5, 0.25], k
        assert len(R.nms_image(an, reg, cls * 0, (128, 128), THR, IOU, kind=k)[0]) == 0
        assert list(R.nms_image(an, reg, cls * (np.arange(5) == 2)[:, None], (128, 128), THR, IOU, kind=k)[0]) == [2]
    # two identical boxes: IoU 1 -> linear weight 0, gaussian weight exp(-2); the second leaves when its score falls to the floor
    an = np.array([[0, 0, 10, 10]] * 2, np.float32)
    cls = np.array([[0.5], [0.25]], np.float32)
    assert len(R.nms_image(an, reg[:2], cls, (128, 128), THR, IOU, kind="soft_linear")[0]) == 1
    _, _, _, s = R.nms_image(an, reg[:2], cls, (128, 128), THR, IOU, kind="soft_gaussian", score_floor=0.01)
    assert list(s) == [np.float32(0.5), np.float32(0.25) * np.float32(np.exp(-2.0))]
    assert len(R.nms_image(an, reg[:2], cls, (128, 128), THR, IOU, kind="soft_gaussian")[0]) == 1         # 0.034 is under the threshold


def test_entry_point_rejects_bad_options_without_a_gpu():
    """the argument checks of hn_det_postprocess_ex come before its first launch; the workspace of the soft kinds has no bit mask"""
    import __graft_entry__ as g
    g.build()
    from multitask_hydranet_amd._lib import lib
    l = lib()
    n, cap = 2, 4096
    assert l.query("hn_det_post_ws_bytes_ex", n, cap, 0) == l.query("hn_det_post_ws_bytes", n, cap) == l.query("hn_det_post_ws_bytes_ex", n, cap, 1)
    front = n * cap * 80 + 2 * n * 4 + 256                                       # two candidate arrays, class-offset boxes, counters
    assert l.query("hn_det_post_ws_bytes_ex", n, cap, 0) == front + n * cap * (cap // 64) * 8
    for kind in (2, 3):
        assert l.query("hn_det_post_ws_bytes_ex", n, cap, kind) == front + n * cap * 9
    f = l.raw("hn_det_postprocess_ex")
    p = 4096                                                                     # any non-null address: a rejected call dereferences nothing
    good = [p, p, p, 2, 100, 3, 128, 128, 0.05, 0.5, 64, p, p, p, p, p, p, 0, 0.5, 0.05, 0, 0]
    for at, bad in ((17, 4), (17, -1), (18, 0.0), (18, -1.0), (18, float("inf")), (18, float("nan")), (20, -1), (10, 0), (10, 32769), (0, None),
                    (11, None), (16, None)):
        args = list(good)
        args[at] = bad
        assert f(*args, None) == 1, (at, bad)
