"""CPU: per-image task masks (gt_dict["task_valid"]).  The masked reference tests/partial_ref.py -- the existing float64 /
integer references applied to the sub-batch of labelled images -- gives the unmasked references themselves under an all-ones mask, zeros
under an all-zeros mask and the sub-batch's numbers in between; the library exports a `_masked` twin of every loss entry point, each of
which rejects a null mask (and the lane pair a row count that does not divide M) before any launch; HydraNet.cal_loss validates the mask
tensor without a GPU."""
import copy
import ctypes

import numpy as np
import pytest
import torch

from tests import det_atss_ref, loss_ref as R, lovasz_ref, partial_ref as P
from tests.helpers import load_cfg

MASKED = ("hn_seg_loss_fwd_masked", "hn_seg_loss_bwd_masked", "hn_seg_loss_bwd_s2d_masked", "hn_seg_focal_fwd_masked", "hn_seg_focal_bwd_masked",
          "hn_seg_lovasz_fwd_masked", "hn_seg_lovasz_bwd_masked", "hn_seg_lovasz_bwd_s2d_masked", "hn_det_loss_fwd_masked",
          "hn_det_loss_fwd_assigned_masked", "hn_det_loss_bwd_masked", "hn_det_loss_iou_fwd_masked", "hn_det_loss_iou_fwd_assigned_masked",
          "hn_det_loss_iou_bwd_masked", "hn_lane_cls_loss_fwd_masked", "hn_lane_cls_loss_bwd_masked")


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from multitask_hydranet_amd import _lib
    return _lib


# ------------------------------------------------------------------------------------------------------------------------------------
# the reference
# ------------------------------------------------------------------------------------------------------------------------------------
def test_all_ones_mask_is_the_unmasked_reference_seg():
    n, h, w, C = 3, 8, 12, 5
    logits, target, cw = R.seg_case(0, C, n, h, w)
    k, _ = R.choose_k(R.seg_ce(logits, target, cw)[0])
    ones = np.ones(n, np.uint8)
    for topk in (0, 1):
        v0, g0 = R.seg_ce_mean(logits, target, cw, topk, k)
        v1, g1 = P.seg_ce_mean(logits, target, cw, topk, k, ones)
        assert v0 == v1 and (g0 == g1).all()
    fl, ft, fcw = R.focal_case(C, m=n * h * w)
    v0, g0 = R.seg_focal(fl, ft, fcw, 2.0, 1.0)
    v1, g1 = P.seg_focal(fl.reshape(n, -1, C), ft.reshape(n, -1), fcw, 2.0, 1.0, ones)
    assert v0 == v1 and (g0.reshape(g1.shape) == g1).all()
    x = torch.from_numpy(logits.reshape(n, h, w, C)).permute(0, 3, 1, 2).contiguous()
    t = torch.from_numpy(np.where((target < 0) | (target >= C), 255, target).reshape(n, h, w))
    xd = x.double().requires_grad_(True)
    val = lovasz_ref.lovasz_softmax_ref(xd, t)
    (g,) = torch.autograd.grad(val, xd)
    v1, g1 = P.seg_lovasz(x, t, ones)
    assert float(val.detach()) == v1 and (g.numpy() == g1).all()


def test_sub_batch_and_empty_mask_seg():
    n, h, w, C = 3, 8, 12, 5
    logits, target, cw = R.seg_case(0, C, n, h, w)
    k, _ = R.choose_k(R.seg_ce(logits, target, cw)[0])
    v, g = P.seg_ce_mean(logits, target, cw, 1, k, [1, 0, 1])
    v0, g0 = R.seg_ce_mean(logits[[0, 2]], target[[0, 2]], cw, 1, k)
    assert v == v0 and (g[[0, 2]] == g0).all() and (g[1] == 0).all()
    v, g = P.seg_ce_mean(logits, target, cw, 1, k, [0, 0, 0])
    assert v == 0.0 and g.shape == logits.shape and (g == 0).all()
    v, g = P.seg_focal(logits, np.clip(target, 0, C - 1), cw, 2.0, 1.0, [0, 0, 0])
    assert v == 0.0 and (g == 0).all()


@pytest.mark.parametrize("kind", ["smooth_l1", "giou", "diou", "ciou"])
def test_all_ones_mask_is_the_unmasked_reference_det(kind):
    N, A, K = 3, 257, 9
    cls, reg, anc, ann = R.det_case(N, A, K)
    got = P.det(cls, reg, anc, ann, np.ones(N, np.uint8), kind, gcls=1.0, greg=50.0)
    sl1 = R.det_smooth_l1(cls, reg, anc, ann, gcls=1.0, greg=50.0)
    assert (got["assign"] == sl1["assign"]).all() and got["npos"] == sl1["npos"]
    if kind == "smooth_l1":                       # the numpy restatement and the torch one given its assignment: two routes to one number
        assert abs(got["cls"] - sl1["cls"]) <= 1e-12 * abs(sl1["cls"]) and abs(got["reg"] - sl1["reg"]) <= 1e-12 * abs(sl1["reg"])
        assert np.abs(got["dcls"] - sl1["dcls"]).max() <= 1e-12 * np.abs(sl1["dcls"]).max()
        assert np.abs(got["dreg"] - sl1["dreg"]).max() <= 1e-12 * np.abs(sl1["dreg"]).max()
    c, r = torch.from_numpy(cls).double(), torch.from_numpy(reg).double()
    o = det_atss_ref.losses_given_assign(c, r, torch.from_numpy(anc).double(), torch.from_numpy(ann).double(), sl1["assign"], kind)
    assert (got["cls"], got["reg"], got["pos_iou"]) == (float(o["cls"]), float(o["reg"]), float(o["pos_iou"]))
    # a mask: image 1 (no boxes in det_case) labelled, image 0 not
    m = P.det(cls, reg, anc, ann, [0, 1, 1], kind)
    assert (m["assign"][0] == -2).all() and m["npos"][0] == 0 and (m["dcls"][0] == 0).all() and (m["dreg"][0] == 0).all()
    o = det_atss_ref.losses_given_assign(c[1:], r[1:], torch.from_numpy(anc).double(), torch.from_numpy(ann[1:]).double(), sl1["assign"][1:], kind)
    assert m["cls"] == float(o["cls"]) and m["reg"] == float(o["reg"])
    z = P.det(cls, reg, anc, ann, [0, 0, 0], kind)
    assert (z["cls"], z["reg"], z["pos_iou"], z["npos"]) == (0.0, 0.0, 0.0, [0, 0, 0]) and (z["assign"] == -2).all() and (z["dcls"] == 0).all()


def test_all_ones_mask_is_the_unmasked_reference_lane():
    rows, N = 128, 3
    for z, t, ratio, _ in R.lane_pattern("ties", N * rows):
        a, b = R.lane_cls(z, t, ratio, 10.0, 1.3, 0.7), P.lane_cls(z, t, rows, np.ones(N, np.uint8), ratio, 10.0, 1.3, 0.7)
        for key in ("pos", "neg", "thr", "posn", "npos", "nneg", "k"):
            assert a[key] == b[key], key
        assert (a["pmask"] == b["pmask"]).all() and (a["dlogits"] == b["dlogits"]).all()
        m = P.lane_cls(z, t, rows, [1, 0, 1], ratio)
        keep = np.r_[0:rows, 2 * rows:3 * rows]
        s = R.lane_cls(z[keep], t[keep], ratio)
        assert (m["pos"], m["neg"], m["npos"], m["nneg"]) == (s["pos"], s["neg"], s["npos"], s["nneg"])
        assert not m["pmask"][rows:2 * rows].any() and (m["dlogits"][rows:2 * rows] == 0).all() and (m["rows"] == keep).all()
        e = P.lane_cls(z, t, rows, [0, 0, 0], ratio)
        assert (e["pos"], e["neg"], e["npos"], e["nneg"], e["posn"]) == (0.0, 0.0, 0, 0, 1) and np.isposinf(e["thr"])
    p, t, pmask, posn = R.lane_loc_case(33, M=3 * 13, wcol=1)
    v0, g0, _ = R.lane_loc(p, t, pmask, posn, 1)
    v1, g1 = P.lane_loc(p, t, 13, [1, 1, 1], pmask, posn, 1)
    assert v0 == v1 and (g0 == g1).all()
    v1, g1 = P.lane_loc(p, t, 13, [0, 0, 0], pmask, posn, 1)
    assert v1 == 0.0 and (g1 == 0).all()


# ------------------------------------------------------------------------------------------------------------------------------------
# the library
# ------------------------------------------------------------------------------------------------------------------------------------
def test_library_exports_the_masked_entry_points_and_checks_their_arguments(built):
    sig = built.parse_header()
    dll = ctypes.CDLL(built.SO_PATH)
    for name in MASKED:
        assert name in sig and hasattr(dll, name), name
        assert name[:-len("_masked")] in sig                                   # every twin has its unmasked entry point
    l = built.lib()
    # HN_CHECK_ARG returns 1 before any launch: the pointers are never dereferenced (1 stands for 'not null'); None is the null mask
    seg = (1, 5, 5, 1, 1, 1, 255, 2)
    assert l.raw("hn_seg_loss_fwd_masked")(*seg, 16, 1, 4, None, 1, 1, None) == 1
    assert l.raw("hn_seg_loss_bwd_masked")(*seg, 16, 1, 4, None, 1, 1, 1, 5, None) == 1
    assert l.raw("hn_seg_loss_bwd_s2d_masked")(*seg, 4, 4, 1, 4, None, 1, 1, 1, 24, None) == 1
    assert l.raw("hn_seg_loss_fwd_masked")(*seg, 16, 1, 17, 1, 1, 1, None) == 1                     # k > HW, as the unmasked call
    focal = (1, 5, 5, 1, 1, 1, 2.0, 1.0, 2, 16)
    assert l.raw("hn_seg_focal_fwd_masked")(*focal, None, 1, 1, None) == 1
    assert l.raw("hn_seg_focal_bwd_masked")(*focal, None, 1, 1, 5, None) == 1
    lov = (1, 5, 5, 1, 1, 255, 2)
    assert l.raw("hn_seg_lovasz_fwd_masked")(*lov, 16, None, 1, 1, None) == 1
    assert l.raw("hn_seg_lovasz_bwd_masked")(*lov, 16, None, 1, 1, 1, 5, None) == 1
    assert l.raw("hn_seg_lovasz_bwd_s2d_masked")(*lov, 4, 4, None, 1, 1, 1, 24, None) == 1
    det = (1, 1, 1, 1, 2, 300, 9, 8)
    for name in ("hn_det_loss_fwd_masked", "hn_det_loss_fwd_assigned_masked"):
        assert l.raw(name)(*det, None, 1, 1, 1, 1, None) == 1
        assert l.raw(name)(1, 1, 1, 1, 2, 300, 33, 8, 1, 1, 1, 1, 1, None) == 1                      # K beyond the bound, as the unmasked call
    assert l.raw("hn_det_loss_bwd_masked")(*det, None, 1, 1, 1, 1, 1, None) == 1
    for name in ("hn_det_loss_iou_fwd_masked", "hn_det_loss_iou_fwd_assigned_masked"):
        assert l.raw(name)(*det, 1, None, 1, 1, 1, 1, None) == 1
        assert l.raw(name)(*det, 4, 1, 1, 1, 1, 1, None) == 1                                        # kind outside 1..3
    assert l.raw("hn_det_loss_iou_bwd_masked")(*det, 1, None, 1, 1, 1, 1, 1, None) == 1
    assert l.raw("hn_det_loss_iou_bwd_masked")(*det, 0, 1, 1, 1, 1, 1, 1, None) == 1
    assert l.raw("hn_lane_cls_loss_fwd_masked")(1, 1, 384, 128, None, 15.0, 10.0, 1, 1, 1, 1, None) == 1
    assert l.raw("hn_lane_cls_loss_bwd_masked")(1, 1, 1, 1, 1, 10.0, 384, 128, None, 1, None) == 1
    for rows in (0, -1, 100, 385):                                                                    # M = 384 is no multiple
        assert l.raw("hn_lane_cls_loss_fwd_masked")(1, 1, 384, rows, 1, 15.0, 10.0, 1, 1, 1, 1, None) == 1, rows
        assert l.raw("hn_lane_cls_loss_bwd_masked")(1, 1, 1, 1, 1, 10.0, 384, rows, 1, 1, None) == 1, rows


def test_ops_take_valid_and_reject_a_malformed_mask(built):
    import inspect
    from multitask_hydranet_amd import ops as K
    for fn in (K.seg_loss_hip, K.seg_focal_loss_hip, K.seg_lovasz_loss_hip, K.det_loss_hip, K.det_iou_loss_hip, K.lane_cls_loss_hip,
               K.lane_loc_loss_hip):
        assert inspect.signature(fn).parameters["valid"].default is None, fn.__name__
    for fn in (K.lane_cls_loss_hip, K.lane_loc_loss_hip):
        assert inspect.signature(fn).parameters["rows_per_image"].default is None
    dev = torch.device("cpu")
    ok = torch.ones(3, dtype=torch.uint8)
    assert K._task_valid_row(ok, 3, dev) is ok
    for bad in (torch.ones(3, dtype=torch.bool), torch.ones(3, dtype=torch.int64), torch.ones(4, dtype=torch.uint8),
                torch.ones(3, 1, dtype=torch.uint8), torch.ones(6, dtype=torch.uint8)[::2], [1, 1, 1]):
        with pytest.raises(ValueError):
            K._task_valid_row(bad, 3, dev)


# ------------------------------------------------------------------------------------------------------------------------------------
# the module
# ------------------------------------------------------------------------------------------------------------------------------------
def test_cal_loss_validates_task_valid(built):
    from multitask_hydranet_amd import HydraNet
    net = HydraNet(copy.deepcopy(load_cfg("hydranet_tiny.yml")))
    n = 2
    pred = {"seg": torch.zeros(n, 5, 4, 4), "detection": {"classification": torch.zeros(n, 6, 2)}, "lane": {"predict_cls": torch.zeros(n, 3, 2)}}
    assert net._task_valid(pred, {}) == {}
    rows = net._task_valid(pred, {"task_valid": torch.tensor([[1, 0], [0, 1], [1, 1]], dtype=torch.uint8)})
    assert sorted(rows) == ["det", "lane", "seg"]
    assert rows["seg"]["valid"].tolist() == [1, 0] and rows["det"]["valid"].tolist() == [0, 1] and rows["lane"]["valid"].tolist() == [1, 1]
    assert all(v["valid"].is_contiguous() and v["valid"].dtype == torch.uint8 for v in rows.values())
    for bad in (torch.ones(3, n, dtype=torch.bool), torch.ones(3, n, dtype=torch.float32), torch.ones(n, 3, dtype=torch.uint8),
                torch.ones(3, n + 1, dtype=torch.uint8), torch.ones(3 * n, dtype=torch.uint8), [[1, 1]] * 3,
                torch.ones(3, n, dtype=torch.uint8, device="meta")):
        with pytest.raises(ValueError, match="task_valid"):
            net.cal_loss(pred, {"task_valid": bad})


# ------------------------------------------------------------------------------------------------------------------------------------
# the dataset
# ------------------------------------------------------------------------------------------------------------------------------------
def _tree(tmp_path, allow):
    """four images at the tiny cfg's network size: `a` without a lane label, `b` without a seg label, `c` without a box label, `d`
    without any"""
    import json
    import os
    from PIL import Image
    cfgs = copy.deepcopy(load_cfg("hydranet_tiny.yml"))
    dl = cfgs["dataloader"]
    h, w = dl["network_input_height"], dl["network_input_width"]
    root = str(tmp_path / "set")
    for d in ("images", "labels_lane", "labels_segmentation", "labels_object", "lists"):
        os.makedirs(os.path.join(root, d))
    g = np.random.default_rng(5)
    paths = []
    for name, (seg, det, lane) in (("a", (1, 1, 0)), ("b", (0, 1, 1)), ("c", (1, 0, 1)), ("d", (0, 0, 0))):
        p = os.path.join(root, "images", name + ".jpg")
        Image.fromarray(g.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(p, quality=90)
        paths.append(p)
        if seg:
            Image.fromarray(g.integers(0, 5, (h, w), dtype=np.uint8)).save(os.path.join(root, "labels_segmentation", name + ".png"))
        if det:
            with open(os.path.join(root, "labels_object", name + ".txt"), "w") as f:
                f.write("2,3,%d,%d,1\n4,4,%d,%d,2\n" % (w // 2, h // 2, w - 2, h - 2))
        if lane:
            with open(os.path.join(root, "labels_lane", name + ".json"), "w") as f:
                json.dump({"shapes": [{"label": "lane", "points": [[w * 0.3, h - 1.0], [w * 0.4, h * 0.5], [w * 0.45, h * 0.2]]}]}, f)
    for lst in ("train.txt", "valid.txt"):
        with open(os.path.join(root, "lists", lst), "w") as f:
            f.write("\n".join(paths) + "\n")
    dl["data_list"] = os.path.join(root, "lists")
    if allow is not None:
        dl["allow_missing_labels"] = allow
    assert all(cfgs["train"][k] for k in ("train_lane", "train_seg", "train_detect"))
    return cfgs, (h, w)


@pytest.mark.parametrize("allow", [None, False])
def test_default_still_raises_on_a_missing_label(tmp_path, allow):
    from multitask_hydranet_amd import dataset as D
    cfgs, _ = _tree(tmp_path, allow)
    ds = D.MultitaskData(cfgs, "train")
    assert len(ds) == 4 and not ds.allow_missing_labels and ds.unlabelled == 0
    for i in range(4):
        with pytest.raises(FileNotFoundError):
            ds[i]


@pytest.mark.parametrize("decode_labels", ["host", "device"])
def test_allow_missing_labels_masks_stand_ins_and_collate(tmp_path, decode_labels):
    from multitask_hydranet_amd import dataset as D
    cfgs, (h, w) = _tree(tmp_path, True)
    ds = D.MultitaskData(cfgs, "train", decode_labels=decode_labels)
    assert ds.allow_missing_labels and len(ds) == 3 and ds.unlabelled == 1
    assert [os_name(p["image_path"]) for p in ds.image_annot_path_pairs] == ["a", "b", "c"]
    items = [ds[i] for i in range(3)]
    assert [it["task_valid"].tolist() for it in items] == [[1, 1, 0], [0, 1, 1], [1, 0, 1]]          # (seg, det, lane)
    assert all(it["task_valid"].dtype == np.uint8 for it in items)
    a, b, c = items
    assert a["lane_raw"] == {"Lines": [], "Labels": []} and len(b["lane_raw"]["Lines"]) == 1 and len(c["lane_raw"]["Lines"]) == 1
    assert c["det_raw"].shape == (0, 5) and c["det_raw"].dtype == np.float64 and a["det_raw"].shape == (2, 5)
    assert b["src_seg"].shape == (h, w) and b["src_seg"].dtype == np.uint8 and (b["src_seg"] == 255).all()  # the already-decoded slot
    assert "src_seg_stream" not in b
    for it in (a, c):
        assert ("src_seg_stream" in it) == (decode_labels == "device") and ("src_seg" in it) == (decode_labels == "host")
    out = ds.collate_fn(items)
    tv = out["task_valid"]
    assert isinstance(tv, np.ndarray) and tv.dtype == np.uint8 and tv.shape == (3, 3) and tv.flags["C_CONTIGUOUS"]
    assert tv.tolist() == [[1, 0, 1], [1, 1, 0], [0, 1, 1]]                                            # rows seg, det, lane
    assert len(out["lane_raw"]) == 3 and len(out["det_raw"]) == 3 and out["det_raw"][2].shape == (0, 5)
    if decode_labels == "device":
        pk = out["src_seg_streams"]
        assert pk["heads"][1] is None and pk["maps"][1].shape == (h, w) and pk["heads"][0] is not None and pk["heads"][2] is not None
    else:
        assert len(out["src_segs"]["shapes"]) == 3
    # a full-labelled set under the switch: all ones, nothing dropped; the default emits no mask at all
    one = ds.collate_fn([items[0]])
    assert one["task_valid"].shape == (3, 1)
    cfgs_off, _ = _tree(tmp_path / "off", None)
    assert "task_valid" not in D.MultitaskData(cfgs_off, "train").image_annot_path_pairs[0]


def test_allow_missing_labels_counts_trained_tasks_only_and_never_splits_without_lanes(tmp_path):
    from multitask_hydranet_amd import augment as A, dataset as D
    cfgs, _ = _tree(tmp_path, True)
    cfgs["train"]["train_detect"] = False
    ds = D.MultitaskData(cfgs, "train")
    assert [p["task_valid"] for p in ds.image_annot_path_pairs] == [(1, 0, 0), (0, 0, 1), (1, 0, 1)] and ds.unlabelled == 1
    cfgs["train"]["train_seg"] = False
    ds = D.MultitaskData(cfgs, "train")                                   # lane only: `a` has no lane label and leaves as well
    assert [os_name(p["image_path"]) for p in ds.image_annot_path_pairs] == ["b", "c"] and ds.unlabelled == 2
    cfgs, _ = _tree(tmp_path / "split", True)
    cfgs["dataloader"].update(with_aug=True, do_split=True)
    calls = []

    def rule(lanes, w, h):
        calls.append(len(lanes["Lines"]))
        return True, 0.25
    ds = D.MultitaskData(cfgs, "train", base_seed=4, split_rule=rule)
    plans = [ds[i]["aug_plan"] for i in range(3)]
    assert calls == [1, 1]                                                # `a` (no lane label) never reaches the rule
    ref = A.sample_plan(4, 0, 0, do_flip=ds.do_flip, do_split=True, split_ratio=None)
    assert plans[0] == ref


def os_name(path):
    import os
    return os.path.splitext(os.path.basename(path))[0]
