"""GPU: the demo on a video (python -m multitask_hydranet_amd.demo --video IN.avi --out OUT.avi).  Demo.process_device_batch gives for every
frame of a batch what Demo.process_device gives for that frame alone (bytes and records); demo.run_video writes, for a Motion-JPEG AVI
built by tests/avi_ref.py's independent muxer (table-less frames and a repeat chunk among them), an AVI that avi_ref's walker reads back
frame by frame as those per-frame results, with either entropy setting and with a chosen output size.  Tiny cfg, recorded weights."""
import io
import json
import os

import numpy as np
import pytest
import torch

from tests import avi_ref as R
from tests.test_demo_images_gpu import make_demo

pytestmark = pytest.mark.gpu

PLAN = [0, 1, 2, 3, 3, 4]                # the clip's chunks: five frames and a repeat chunk after frame 3


@pytest.fixture(scope="module")
def demo():
    return make_demo()


@pytest.fixture(scope="module")
def singles(demo):
    """Demo.process_device on every frame of the clip alone: the reference of every test here, computed once"""
    from multitask_hydranet_amd import jpeg
    out = []
    for data in R.clip()[1]:
        r = demo.process_device(jpeg.imread_bgr_device(data, device=demo.device))
        out.append({"jpeg": r["jpeg"], "lanes": r["lanes"][0], "detections": r["detections"][0]})
    drawn = sum(len(s["lanes"]) + len(s["detections"]["rois"]) for s in out)
    assert drawn > 0, "the thresholds let nothing through: the drawing stages were not exercised"
    return out


@pytest.fixture(scope="module")
def clip_avi(tmp_path_factory):
    stored, _ = R.clip()
    items = [(b"00dc", f) for f in stored[:4]] + [(b"00dc", b""), (b"00dc", stored[4])]
    data, spans = R.mux(items, R.CLIP_W, R.CLIP_H, 30000, 1001, audio=True)
    path = tmp_path_factory.mktemp("video") / "clip.avi"
    path.write_bytes(data)
    return str(path)


@pytest.fixture(scope="module")
def host_run(demo, clip_avi, tmp_path_factory):
    from multitask_hydranet_amd import demo as DM
    dst = str(tmp_path_factory.mktemp("video_out") / "clip_vis.avi")
    summary = DM.run_video(demo, clip_avi, dst, batch=2)
    return dst, summary


def same_detections(a, b):
    return all(np.array_equal(np.asarray(a[k]), np.asarray(b[k])) for k in ("rois", "class_ids", "scores")) and set(a) == set(b)


@pytest.mark.parametrize("B", [5, 2])
def test_batch_equals_the_frames_alone(demo, singles, B):
    from multitask_hydranet_amd import jpeg
    frames = jpeg.imread_bgr_device(list(R.clip()[1][:B]), device=demo.device)
    r = demo.process_device_batch(frames)
    assert len(r["jpeg"]) == len(r["lanes"]) == len(r["detections"]) == B and r["org_size"] == (R.CLIP_W, R.CLIP_H)
    assert r["visual"]["data"].is_cuda and r["visual"]["shapes"].tolist() == [[R.CLIP_H, R.CLIP_W]] * B
    drawn = 0
    for t in range(B):
        print("frame %d of %d: %d lanes, %d boxes, jpeg identical: %s" % (t, B, len(r["lanes"][t]), len(r["detections"][t]["rois"]), r["jpeg"][t] == singles[t]["jpeg"]))
        assert r["lanes"][t] == singles[t]["lanes"]
        assert same_detections(r["detections"][t], singles[t]["detections"])
        assert r["jpeg"][t] == singles[t]["jpeg"]
        drawn += len(r["lanes"][t]) + len(r["detections"][t]["rois"])
    assert drawn > 0, "the thresholds let nothing through: the drawing stages were not exercised"


def test_run_video_groups_of_two(host_run, singles):
    from PIL import Image
    dst, summary = host_run
    got = R.walk(open(dst, "rb").read())
    assert len(got["frames"]) == 6 and got["avih_frames"] == got["strh_length"] == 6
    assert (got["width"], got["height"], got["rate"], got["scale"]) == (R.CLIP_W, R.CLIP_H, 30000, 1001)
    for i, t in enumerate(PLAN):
        assert got["frames"][i] == singles[t]["jpeg"], "output frame %d is not process_device's result for frame %d" % (i, t)
        with Image.open(io.BytesIO(got["frames"][i])) as im:
            assert im.format == "JPEG" and im.size == (R.CLIP_W, R.CLIP_H)
            im.load()
    assert got["frames"][4] == got["frames"][3]                          # the repeat chunk
    res = json.load(open(dst + ".results.json"))
    assert len(res) == len(summary) == 6 and [e["frame"] for e in res] == list(range(6))
    assert set(res[0]) == {"frame", "file", "ms", "lanes", "boxes"}
    for e, t in zip(res, PLAN):
        assert e["lanes"] == len(singles[t]["lanes"]) and e["boxes"] == len(singles[t]["detections"]["rois"])


def test_run_video_with_both_entropy_stages_on_the_device(demo, clip_avi, host_run, tmp_path):
    """the same bytes, the table-less frames through the device's Huffman stage included"""
    from multitask_hydranet_amd import demo as DM
    dst = str(tmp_path / "dev.avi")
    DM.run_video(demo, clip_avi, dst, batch=2, entropy="device", decode_entropy="device")
    assert open(dst, "rb").read() == open(host_run[0], "rb").read()


def test_run_video_at_a_chosen_size(demo, clip_avi, tmp_path):
    from PIL import Image
    from multitask_hydranet_amd import demo as DM
    from multitask_hydranet_amd import jpeg, jpeg_encode
    from multitask_hydranet_amd.preprocess import resize_bgr
    dst = str(tmp_path / "small.avi")
    DM.run_video(demo, clip_avi, dst, batch=2, size=(1280, 720))
    got = R.walk(open(dst, "rb").read())
    assert len(got["frames"]) == 6 and (got["width"], got["height"], got["rate"], got["scale"]) == (1280, 720, 30000, 1001)
    want = []
    full = R.clip()[1]
    for group in ((0, 1), (2, 3), (4,)):                                 # the unresized run, its annotated frames resized and encoded by hand
        r = demo.process_device_batch(jpeg.imread_bgr_device([full[t] for t in group], device=demo.device))
        want += jpeg_encode.encode_batch(resize_bgr(r["visual"], (720, 1280)))
    for i, t in enumerate(PLAN):
        assert got["frames"][i] == want[t], (i, t)
        with Image.open(io.BytesIO(got["frames"][i])) as im:
            assert im.format == "JPEG" and im.size == (1280, 720)


def test_max_frames(demo, clip_avi, host_run, tmp_path):
    from multitask_hydranet_amd import demo as DM
    dst = str(tmp_path / "five.avi")
    summary = DM.run_video(demo, clip_avi, dst, batch=8, max_frames=5)
    got, ref = R.walk(open(dst, "rb").read()), R.walk(open(host_run[0], "rb").read())
    assert len(summary) == 5 and got["frames"] == ref["frames"][:5]      # one group of four coded frames and the repeat chunk


def test_command_line(clip_avi, tmp_path, capsys):
    from multitask_hydranet_amd import demo as DM
    cfg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cfgs", "hydranet_tiny.yml")
    with pytest.raises(SystemExit) as e:
        DM.main(["--cfg", cfg, "--video", clip_avi])
    assert e.value.code == 2 and "--video needs --out" in capsys.readouterr().err
    dst = str(tmp_path / "cli.avi")
    summary = DM.main(["--cfg", cfg, "--video", clip_avi, "--out", dst, "--batch", "2", "--size", "640x360", "--max-frames", "3"])
    got = R.walk(open(dst, "rb").read())
    assert len(summary) == 3 and len(got["frames"]) == 3 and (got["width"], got["height"]) == (640, 360)
    assert os.path.exists(dst + ".results.json")
