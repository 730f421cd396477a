"""Host half of the device augmentation (augment.py, dataset.py): plan distribution, affine composition, label transforms, the numpy
restatement's known answers and MultitaskData on a tiny tree in the reference's layout."""
import json
import math
import os

import numpy as np
import pytest

import augment_ref as R
from multitask_hydranet_amd import augment as A
from multitask_hydranet_amd import dataset as D


def _within(count, n, p, z=5.0):
    sd = math.sqrt(n * p * (1 - p))
    return abs(count - n * p) <= z * sd + 1


def test_plan_frequencies():
    n = 20000
    plans = [A.sample_plan(7, 3, i) for i in range(n)]
    photo = [p["photo"] for p in plans if p["photo"] is not None]
    geom = [p["geom"] for p in plans if p["geom"]]
    assert _within(len(photo), n, 0.6) and _within(len(geom), n, 0.6)
    for op in A.PHOTO_OPS[1:]:
        assert _within(sum(p["op"] == op for p in photo), len(photo), 1 / 7), op
    mul = [p for p in photo if p["op"] == "multiply"]
    assert _within(sum(p["per_channel"] for p in mul), len(mul), 0.2)
    noi = [p for p in photo if p["op"] == "noise"]
    assert _within(sum(p["per_channel"] for p in noi), len(noi), 0.5)
    assert all(0 <= p["scale"] <= 25.5 for p in noi)
    assert all(0.5 <= p["sigma"] <= 1.5 for p in photo if p["op"] == "blur")
    subsets = {}
    for g in geom:
        assert len(g) == 4
        subsets[tuple(x[0] for x in g)] = subsets.get(tuple(x[0] for x in g), 0) + 1
    assert len(subsets) == 5
    for k, c in subsets.items():
        assert _within(c, len(geom), 0.2), k
        order = ["fliplr", "translate_x", "shear_x", "rotate", "crop"]
        assert list(k) == sorted(k, key=order.index)
    crops = [x[1] for g in geom for x in g if x[0] == "crop"]
    for j, vals in ((0, (0.0, 0.2)), (1, (0.0, 0.15)), (3, (0.0, 0.15))):
        assert set(c[j] for c in crops) == set(vals)
        assert _within(sum(c[j] == vals[1] for c in crops), len(crops), 0.5)
    assert all(c[2] == 0.0 for c in crops)
    tr = [x[1] for g in geom for x in g if x[0] == "translate_x"]
    assert min(tr) == -16 and max(tr) == 16 and all(isinstance(t, int) for t in tr)


def test_plan_flipud_and_identity():
    plans = [A.sample_plan(1, 0, i, do_flip=True) for i in range(3000)]
    names = set(x[0] for p in plans for x in p["geom"])
    assert "flipud" in names
    assert len(set(tuple(x[0] for x in p["geom"]) for p in plans if p["geom"])) == 15
    assert A.sample_plan(1, 0, 5, with_aug=False) == A.identity_plan()
    with pytest.raises(NotImplementedError):
        A.sample_plan(1, 0, 5, do_split=True)
    assert A.sample_plan(3, 1, 9) == A.sample_plan(3, 1, 9) and A.sample_plan(3, 1, 9) != A.sample_plan(3, 2, 9)


def test_forward_matrix_is_product():
    W, H = 1283, 721
    for i in range(200):
        p = A.sample_plan(11, 0, i, do_flip=i % 2 == 0)
        M = np.eye(3)
        for name, param in p["geom"]:
            M = R.op_matrix(name, param, W, H) @ M
        np.testing.assert_allclose(A.forward_matrix(p, W, H), M, rtol=0, atol=1e-9)


def test_known_answers_boxes_lanes():
    W, H = 100, 50
    F = A.forward_matrix({"geom": [("fliplr", None)]}, W, H)
    np.testing.assert_allclose(A.transform_boxes(np.array([[10, 5, 30, 20, 2]]), F, W, H), [[70, 5, 90, 20, 2]])
    crop = ("crop", (0.2, 0.15, 0.0, 0.15))
    F = A.forward_matrix({"geom": [crop]}, W, H)
    L, T, Rr = round(0.15 * W), round(0.2 * H), round(0.15 * W)
    corners = np.array([[L, T, 1], [W - Rr, H, 1]], dtype=np.float64).T
    np.testing.assert_allclose((F @ corners)[:2].T, [[0, 0], [W, H]], atol=1e-12)
    F = A.forward_matrix({"geom": [("translate_x", 16)]}, W, H)
    out = A.transform_boxes(np.array([[90, 5, 99, 20, 0], [0, 0, 10, 10, 1]]), F, W, H)
    np.testing.assert_allclose(out, [[16, 0, 26, 10, 1]])                     # the first box leaves the frame
    F = A.forward_matrix({"geom": [("translate_x", -16)]}, W, H)
    lane = A.transform_lanes({"Lines": [[{"x": 10.7, "y": 3.9}, {"x": 30.2, "y": 40.0}]], "Labels": ["a"]}, F)
    assert lane["Lines"][0] == [{"x": -5.0, "y": 3.0}, {"x": 14.0, "y": 40.0}]     # -5.3 truncates toward 0
    padded = A.pad_boxes([np.zeros((0, 5)), np.array([[10.0, 10, 20, 20, 1]])], [(0.5, 2.0), (0.5, 2.0)])
    assert padded.shape == (2, 1, 5) and (padded[0] == -1).all()
    np.testing.assert_allclose(padded[1, 0], [5, 20, 10, 40, 1])
    assert A.pad_boxes([np.zeros((0, 5))], [(1, 1)]).shape == (1, 1, 5)


def test_inter_area_known_answers():
    img = np.arange(6 * 4, dtype=np.uint8).reshape(4, 6, 1) * 10
    out = R.inter_area(img, 2, 3)                         # 2x2 blocks: the rounded block mean
    exp = np.rint(img.reshape(2, 2, 3, 2, 1).astype(np.float64).mean(axis=(1, 3)))
    np.testing.assert_array_equal(out, exp)
    rng = np.random.default_rng(0)
    src = rng.integers(0, 256, (1080, 16, 3)).astype(np.uint8)
    out = R.inter_area(src, 640, 16)
    # 1080 -> 640: each output row is the mean of the source interval [1.6875 y, 1.6875 (y + 1)), with fractional edge weights
    s = 1080 / 640
    ref = np.zeros((640, 16, 3))
    for y in range(640):
        a, b = y * s, (y + 1) * s
        for k in range(int(math.floor(a)), min(int(math.ceil(b)), 1080)):
            ref[y] += src[k] * (min(b, k + 1) - max(a, k)) / s
    assert np.abs(out.astype(np.float64) - ref).max() <= 0.5 + 1e-3
    with pytest.raises(ValueError):
        R.inter_area(src, 2000, 16)


def test_philox_known_answer():
    # Random123 kat_vectors, philox4x32_10
    z = R.philox4x32_10(np.zeros((1, 4), np.uint32), (0, 0))[0]
    assert [int(v) for v in z] == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    c = np.array([[0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344]], np.uint32)
    z = R.philox4x32_10(c, (0xa4093822, 0x299f31d0))[0]
    assert [int(v) for v in z] == [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]


def _write_tree(root, sizes, cfg_h=64, cfg_w=96):
    from PIL import Image
    for sub in ("images", "labels_lane", "labels_segmentation", "labels_object"):
        os.makedirs(os.path.join(root, sub), exist_ok=True)
    paths = []
    for i, (w, h) in enumerate(sizes):
        p = os.path.join(root, "images", "f%d.jpg" % i)
        img = np.zeros((h, w, 3), np.uint8)
        img[..., 0] = 250                                           # pure red (RGB) -> BGR[2] = 250
        Image.fromarray(img).save(p, quality=100)
        json.dump({"shapes": [{"label": "solid", "points": [[1.5, 2.5], [10, 40]]}]},
                  open(p.replace(".jpg", ".json").replace("images", "labels_lane"), "w"))
        seg = (np.arange(h * w).reshape(h, w) % 3).astype(np.uint8)
        Image.fromarray(seg).save(p.replace(".jpg", ".png").replace("images", "labels_segmentation"))
        open(p.replace(".jpg", ".txt").replace("images", "labels_object"), "w").write("10,20,30,40,2\n5,5,5,9,1\n")
        paths.append(p)
    for name in ("train.txt", "valid.txt"):
        open(os.path.join(root, name), "w").write("\n".join(paths) + "\n")
    return {"dataloader": {"network_input_width": cfg_w, "network_input_height": cfg_h, "with_aug": True, "do_split": False,
                           "do_flip": False, "data_list": root},
            "train": {"train_lane": True, "train_seg": True, "train_detect": True}}


def test_multitask_data_tree(tmp_path):
    cfgs = _write_tree(str(tmp_path), [(128, 80), (100, 70)])
    ds = D.MultitaskData(cfgs, "train", base_seed=5)
    assert len(ds) == 2
    it = ds[0]
    assert it["src_frame"].shape == (80, 128, 3) and it["src_frame"].dtype == np.uint8
    assert it["src_frame"][..., 2].min() > 240 and it["src_frame"][..., 0].max() < 10       # BGR order
    assert it["lane_raw"] == {"Lines": [[{"x": 1.5, "y": 2.5}, {"x": 10, "y": 40}]], "Labels": ["solid"]}
    np.testing.assert_array_equal(it["det_raw"], [[10, 20, 30, 40, 1]])                      # zero-width box dropped, id - 1
    np.testing.assert_array_equal(it["src_seg"], (np.arange(80 * 128).reshape(80, 128) % 3))
    assert it["aug_plan"] == A.sample_plan(5, 0, 0)
    b = ds.collate_fn([ds[0], ds[1]])
    assert b["src_frames"]["shapes"].tolist() == [[80, 128], [70, 100]] and "image" not in b
    assert int(b["src_frames"]["offsets"][1]) == 80 * 128 * 3
    assert D.MultitaskData(cfgs, "val")[0]["aug_plan"] == A.identity_plan()
    small = _write_tree(str(tmp_path / "s"), [(50, 40)])
    with pytest.raises(ValueError):
        D.MultitaskData(small, "train")[0]
    cfgs["dataloader"]["do_split"] = True
    with pytest.raises(NotImplementedError):
        D.MultitaskData(cfgs, "train")


def test_plans_independent_of_workers(tmp_path):
    import torch
    cfgs = _write_tree(str(tmp_path), [(128, 80)] * 6)
    ds = D.MultitaskData(cfgs, "train", base_seed=9)
    ds.set_epoch(2)
    got = []
    for nw in (0, 2):
        dl = torch.utils.data.DataLoader(ds, batch_size=2, shuffle=False, num_workers=nw, collate_fn=ds.collate_fn)
        got.append([p for b in dl for p in b["aug_plans"]])
    assert got[0] == got[1] == [A.sample_plan(9, 2, i) for i in range(6)]


def test_descriptor_layout():
    assert A.DESC_DTYPE.itemsize == 176
    d = np.zeros(2, dtype=A.DESC_DTYPE)
    e = d[1]
    e["Hs"], e["ws_off"] = 7, -1
    assert d[1]["Hs"] == 7 and d[1]["ws_off"] == -1
    r, w = A.blur_weights(1.5)
    assert r == 5 and abs(float(w[0] + 2 * w[1:].sum()) - 1) < 1e-6
    assert A.blur_weights(0.5)[0] == 2
