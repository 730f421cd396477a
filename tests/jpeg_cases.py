"""Shared by tests/test_jpeg_cpu.py and tests/test_jpeg_gpu.py: the matrix of JPEG streams written at test time with PIL's own encoder
from seeded images, the committed sample frames, and a data-list tree over them."""
import io
import json
import os
import zlib

import numpy as np

from tests.helpers import GOLD

SUBSAMPLINGS = ("4:4:4", "4:2:2", "4:2:0", "grey")
QUALITIES = (50, 75, 95)
SIZES = ((1, 1), (8, 8), (17, 33), (157, 66), (640, 360), (1570, 660))          # width x height
# (sub-sampling, quality, optimize, (W, H), restart_marker_blocks): the whole matrix, plus restart intervals on the 4:2:0 and greyscale streams
MATRIX = [(ss, q, opt, size, 0) for ss in SUBSAMPLINGS for q in QUALITIES for opt in (False, True) for size in SIZES]
MATRIX += [(ss, q, opt, size, 4) for ss in ("4:2:0", "grey") for q in QUALITIES for opt in (False, True) for size in SIZES]
GOLDEN_FRAMES = ("frame_2560x1440.jpg", "frame_1570x660.jpg", "frame_1920x1080.jpg")


def case_id(case):
    ss, q, opt, (w, h), rst = case
    return "%s-q%d-%s-%dx%d%s" % (ss.replace(":", ""), q, "opt" if opt else "std", w, h, "-rst%d" % rst if rst else "")


def seeded_image(w, h, seed):
    """smooth gradients + noise + hard edges (saturated rectangles), so high-frequency coefficients and the range limiter are exercised"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    a = np.stack([x * 255.0 / max(1, w - 1), y * 255.0 / max(1, h - 1), ((x + 2 * y) * 3.0) % 256], 2)
    a += rng.normal(0.0, 25.0, a.shape)
    for _ in range(4):
        y0, x0 = int(rng.integers(0, h)), int(rng.integers(0, w))
        a[y0:y0 + max(1, h // 4), x0:x0 + max(1, w // 3)] = rng.integers(0, 2, 3) * 255.0
    return np.clip(a, 0, 255).astype(np.uint8)


def encode(case):
    """the case's JPEG bytes, written by PIL"""
    from PIL import Image
    ss, q, opt, (w, h), rst = case
    a = seeded_image(w, h, zlib.crc32(case_id(case).encode()))
    im = Image.fromarray(a[..., 0] if ss == "grey" else a)
    kw = dict(quality=q, optimize=opt)
    if ss != "grey":
        kw["subsampling"] = ss
    if rst:
        kw["restart_marker_blocks"] = rst
    bio = io.BytesIO()
    im.save(bio, "JPEG", **kw)
    data = bio.getvalue()
    if rst:
        assert b"\xff\xdd\x00\x04" in data, "the encoder wrote no DRI segment"
    return data


def pil_bgr(data):
    from PIL import Image
    return np.ascontiguousarray(np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))[..., ::-1])


def golden_bytes(name):
    with open(os.path.join(GOLD, "jpeg", name), "rb") as f:
        return f.read()


def write_tree(root, images, net_hw):
    """a data-list tree in the reference's layout over `images` ([(file name, encoded bytes)]) with synthetic lane / box / label files ->
    the dataloader + train sections of a cfg"""
    from PIL import Image
    for sub in ("images", "labels_lane", "labels_segmentation", "labels_object"):
        os.makedirs(os.path.join(root, sub), exist_ok=True)
    paths = []
    for i, (name, data) in enumerate(images):
        p = os.path.join(root, "images", name)
        with open(p, "wb") as f:
            f.write(data)
        with Image.open(io.BytesIO(data)) as im:
            w, h = im.size
        json.dump({"shapes": [{"label": "solid", "points": [[0.2 * w + 7 * i, h - 1.0], [0.4 * w, 0.6 * h], [0.5 * w, 0.35 * h]]},
                              {"label": "dash", "points": [[0.9 * w, h - 2.0], [0.7 * w, 0.55 * h], [0.6 * w, 0.4 * h]]}]},
                  open(p.replace(".jpg", ".json").replace("images", "labels_lane"), "w"))
        seg = ((np.arange(h)[:, None] // 37 + np.arange(w)[None, :] // 53 + i) % 3).astype(np.uint8)
        Image.fromarray(seg).save(p.replace(".jpg", ".png").replace("images", "labels_segmentation"))
        with open(p.replace(".jpg", ".txt").replace("images", "labels_object"), "w") as f:
            f.write("%d,%d,%d,%d,2\n%d,%d,%d,%d,1\n" % (w // 10, h // 8, w // 3, h // 2, w // 2, h // 3, w - 5, h - 9))
        paths.append(p)
    for name in ("train.txt", "valid.txt"):
        with open(os.path.join(root, name), "w") as f:
            f.write("\n".join(paths) + "\n")
    return {"dataloader": {"network_input_width": net_hw[1], "network_input_height": net_hw[0], "with_aug": True, "do_split": False,
                           "do_flip": False, "data_list": root},
            "train": {"train_lane": True, "train_seg": True, "train_detect": True}}
