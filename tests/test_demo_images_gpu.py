"""GPU: the demo on image files (python -m multitask_hydranet_amd.demo --images DIR --out DIR_VIS): one annotated JPEG per input, of the
input's name and size, byte for byte the composition of the separately tested stages run by hand -- jpeg.imread_bgr_device ->
preprocess_bgr -> forward -> lane decode + visual -> seg overlay -> det decode + display -> jpeg_encode.  Tiny cfg, recorded weights."""
import io
import json
import os

import numpy as np
import pytest
import torch

from tests import jpeg_cases as C
from tests.helpers import load_cfg, load_npz, tiny_state

pytestmark = pytest.mark.gpu


def make_demo():
    from multitask_hydranet_amd.demo import Demo
    demo = Demo(load_cfg("hydranet_tiny.yml"), fold_batchnorm=False)
    demo.net.load_state_dict(tiny_state(load_npz("tiny_hydranet.npz")))
    demo.net.eval().prepare_inference()
    demo.lane_conf, demo.det_conf = 0.3, 0.3                            # thresholds that let the tiny model produce lanes and boxes
    return demo


def by_hand(demo, data):
    """the stages one by one, each through its own public entry point, frames crossing the host between them"""
    from multitask_hydranet_amd import draw, jpeg, jpeg_encode
    from multitask_hydranet_amd.preprocess import preprocess_bgr
    net = demo.net
    frame = C.pil_bgr(data)                                              # = jpeg.imread_bgr_device (tests/test_jpeg_gpu.py)
    h, w = frame.shape[:2]
    img = preprocess_bgr(frame, (demo.net_h, demo.net_w), device=demo.device)
    with torch.no_grad():
        out = net(img)
    nms = net.laneheader.decode(out["lane"]["predict_cls"][0], out["lane"]["predict_loc"][0], demo.lane_coder, demo.lane_conf, demo.lane_nms, False)
    lanes = net.laneheader.scale_to_org(nms, demo.net_w, demo.net_h, w, h)["Lines"]
    imgs = net.laneheader.visual([frame.copy()], [lanes], w, filter_vertical=True)
    imgs = net.segheader.decode(imgs, out["seg"], (w, h), demo.colors)
    det = net.detectheader.decode(img, out["detection"]["regression"], out["detection"]["classification"], out["detection"]["anchors"],
                                  conf_thres=demo.det_conf, iou_thres=demo.det_iou)
    imgs = net.detectheader.display(det, imgs, demo.obj_list, (w, h), (demo.net_w, demo.net_h))
    return jpeg_encode.encode_batch([imgs[0]], 95, "4:2:0")[0], lanes, det, imgs[0]


def test_demo_over_a_folder_of_jpegs(tmp_path):
    from multitask_hydranet_amd import demo as DM
    src, dst = tmp_path / "images", tmp_path / "images_vis"
    src.mkdir()
    names = {"b_frame.jpg": "frame_1570x660.jpg", "a_frame.jpeg": "frame_1920x1080.jpg", "c_frame.JPG": "frame_2560x1440.jpg"}
    for name, gold in names.items():
        (src / name).write_bytes(C.golden_bytes(gold))
    (src / "notes.txt").write_text("not an image")
    demo = make_demo()
    summary = DM.run_images(demo, str(src), str(dst))
    assert [s["file"] for s in summary] == sorted(names)                 # sorted order, the other file ignored
    assert sorted(os.listdir(dst)) == sorted(list(names) + ["results.json"])
    assert [s["file"] for s in json.load(open(dst / "results.json"))] == sorted(names)
    drawn = 0
    for s in summary:
        data = C.golden_bytes(names[s["file"]])
        got = (dst / s["file"]).read_bytes()
        want, lanes, det, vis = by_hand(demo, data)
        from PIL import Image
        with Image.open(io.BytesIO(got)) as im, Image.open(io.BytesIO(data)) as im0:
            assert im.size == im0.size and im.format == "JPEG"
        assert s["lanes"] == len(lanes) and s["boxes"] == sum(len(d["rois"]) for d in det)
        print("demo %s: %d bytes, %d lanes, %d boxes, identical to the stages by hand: %s" % (s["file"], len(got), s["lanes"], s["boxes"], got == want))
        assert got == want
        assert np.array_equal(C.pil_bgr(got), C.pil_bgr(want))
        drawn += s["lanes"] + s["boxes"]
    assert drawn > 0, "the thresholds let nothing through: the drawing stages were not exercised"


def test_process_device_keeps_the_frame_on_the_device():
    from multitask_hydranet_amd import jpeg
    demo = make_demo()
    data = C.golden_bytes("frame_1570x660.jpg")
    r = demo.process_device(jpeg.imread_bgr_device(data, device=demo.device))
    assert r["visual"]["data"].is_cuda and r["visual"]["shapes"].tolist() == [[660, 1570]] and r["org_size"] == (1570, 660)
    want, lanes, det, vis = by_hand(demo, data)
    assert r["jpeg"] == want
    assert np.array_equal(r["visual"]["data"].cpu().numpy()[:vis.size].reshape(vis.shape), vis)


def test_frames_mode_returns_what_it_returned(tmp_path):
    """--frames: the blended frames without drawing, written as .npy, as before"""
    from multitask_hydranet_amd import demo as DM
    from multitask_hydranet_amd.visual import seg_decode
    from multitask_hydranet_amd.preprocess import preprocess_bgr
    demo = make_demo()
    frame = DM.synthetic_frames(1, 270, 480, seed=4)[0]
    r = demo.process(frame)
    assert set(r) == {"org_size", "lanes", "detections", "visual", "ms"} and isinstance(r["visual"], np.ndarray)
    with torch.no_grad():
        out = demo.net(preprocess_bgr(frame, (demo.net_h, demo.net_w)))
    assert np.array_equal(r["visual"], seg_decode([frame], out["seg"], (480, 270), demo.colors)[0])
    np.save(tmp_path / "frames.npy", DM.synthetic_frames(2, 270, 480, seed=4))
    cfg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cfgs", "hydranet_tiny.yml")
    summary = DM.main(["--cfg", cfg, "--frames", str(tmp_path / "frames.npy"), "--out", str(tmp_path / "out")])
    assert len(summary) == 2 and sorted(os.listdir(tmp_path / "out")) == ["frame_0000.npy", "frame_0001.npy", "results.json"]
    assert np.load(tmp_path / "out" / "frame_0000.npy").shape == (270, 480, 3)
