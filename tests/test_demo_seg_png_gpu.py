"""GPU: the demo's seg class maps as label PNGs (Demo.process_device / process_device_batch with seg_png=True, run_images(seg_dir=), the
command line's --save-seg / --seg-palette).  The PNG decodes to the nearest-resized arg-max of that frame's seg logits, the batch gives
what the frames give alone, and everything the calls returned before is byte for byte what they return with the option off.  Tiny cfg,
recorded weights."""
import io
import os

import numpy as np
import pytest
import torch
import yaml
from PIL import Image

from tests import avi_ref
from tests import png_enc_ref as R
from tests.test_demo_images_gpu import make_demo
from tests.test_demo_video_gpu import same_detections

pytestmark = pytest.mark.gpu

TINY = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cfgs", "hydranet_tiny.yml")


@pytest.fixture(scope="module")
def demo():
    return make_demo()


def png_map(data):
    with Image.open(io.BytesIO(data)) as im:
        return im.mode, np.asarray(im).copy(), im.getpalette()


def expected_map(demo, frames, k=0):
    """the arg-max of frame k's seg logits, nearest-resized to the frame's size with the float64 index rule"""
    from multitask_hydranet_amd import ops as K
    from multitask_hydranet_amd.preprocess import preprocess_bgr
    h, w = (int(v) for v in frames["shapes"][k])
    o = int(frames["offsets"][k])
    frame = frames["data"][o:o + h * w * 3].view(1, h, w, 3)
    with torch.no_grad():
        seg = demo.net(preprocess_bgr(frame, (demo.net_h, demo.net_w), device=demo.device))["seg"]
    mask = K.argmax_channels(seg.detach().float())[0].cpu().numpy()
    return R.resize(mask, (h, w)).astype(np.uint8)


def test_process_device_seg_png(demo):
    from multitask_hydranet_amd import jpeg
    from multitask_hydranet_amd.demo import seg_palette
    data = avi_ref.clip()[1][0]
    want = expected_map(demo, jpeg.imread_bgr_device(data, device=demo.device))
    print("classes in the frame's map:", np.unique(want).tolist())
    off = demo.process_device(jpeg.imread_bgr_device(data, device=demo.device))
    on = demo.process_device(jpeg.imread_bgr_device(data, device=demo.device), seg_png=True)
    assert "seg_png" not in off and set(on) == set(off) | {"seg_png"}
    assert on["jpeg"] == off["jpeg"] and on["lanes"] == off["lanes"] and same_detections(on["detections"][0], off["detections"][0])
    mode, arr, _ = png_map(on["seg_png"])
    assert mode == "L" and arr.shape == (avi_ref.CLIP_H, avi_ref.CLIP_W) and np.array_equal(arr, want)
    pal = demo.process_device(jpeg.imread_bgr_device(data, device=demo.device), seg_png=True, seg_palette=seg_palette(demo.colors))
    mode, arr, table = png_map(pal["seg_png"])
    assert mode == "P" and np.array_equal(arr, want) and pal["jpeg"] == off["jpeg"]
    assert table[3:6] == [128, 0, 128] and table[9:12] == [255, 255, 0]    # the demo's BGR colours as RGB


def test_process_device_batch_seg_png(demo):
    from multitask_hydranet_amd import jpeg
    clip = list(avi_ref.clip()[1][:3])
    off = demo.process_device_batch(jpeg.imread_bgr_device(clip, device=demo.device))
    on = demo.process_device_batch(jpeg.imread_bgr_device(clip, device=demo.device), seg_png=True)
    assert "seg_png" not in off and len(on["seg_png"]) == 3
    assert on["jpeg"] == off["jpeg"] and on["lanes"] == off["lanes"]
    assert all(same_detections(a, b) for a, b in zip(on["detections"], off["detections"]))
    for k in range(3):
        alone = demo.process_device(jpeg.imread_bgr_device(clip[k], device=demo.device), seg_png=True)
        assert on["seg_png"][k] == alone["seg_png"], k
        mode, arr, _ = png_map(on["seg_png"][k])
        assert mode == "L" and np.array_equal(arr, expected_map(demo, jpeg.imread_bgr_device(clip[k], device=demo.device))), k
    small = demo.process_device_batch(jpeg.imread_bgr_device(clip, device=demo.device), out_hw=(90, 160), seg_png=True)
    assert small["seg_png"] == on["seg_png"]                              # the class maps keep the frames' original size


def write_jpegs(folder):
    from multitask_hydranet_amd import demo as DM
    folder.mkdir()
    sizes = {"a.jpg": (300, 400), "b.jpg": (270, 480), "c.jpeg": (300, 400)}
    for k, (name, (h, w)) in enumerate(sizes.items()):
        bgr = DM.synthetic_frames(1, h, w, seed=k)[0]
        Image.fromarray(bgr[:, :, ::-1].copy()).save(str(folder / name), format="JPEG", quality=90)
    return sizes


def test_run_images_writes_the_class_maps(demo, tmp_path):
    from multitask_hydranet_amd import demo as DM
    from multitask_hydranet_amd import jpeg
    sizes = write_jpegs(tmp_path / "images")
    plain = DM.run_images(demo, str(tmp_path / "images"), str(tmp_path / "vis0"))
    summary = DM.run_images(demo, str(tmp_path / "images"), str(tmp_path / "vis"), seg_dir=str(tmp_path / "seg"))
    assert [s["file"] for s in summary] == sorted(sizes) == [s["file"] for s in plain]
    assert sorted(os.listdir(tmp_path / "seg")) == ["a.png", "b.png", "c.png"]
    for name, (h, w) in sizes.items():
        assert (tmp_path / "vis" / name).read_bytes() == (tmp_path / "vis0" / name).read_bytes()
        mode, arr, _ = png_map((tmp_path / "seg" / (os.path.splitext(name)[0] + ".png")).read_bytes())
        want = expected_map(demo, jpeg.imread_bgr_device(str(tmp_path / "images" / name), device=demo.device))
        assert mode == "L" and arr.shape == (h, w) and np.array_equal(arr, want), name


def test_command_line_save_seg(tmp_path):
    from multitask_hydranet_amd import demo as DM
    write_jpegs(tmp_path / "images")
    DM.main(["--cfg", TINY, "--images", str(tmp_path / "images"), "--out", str(tmp_path / "vis"), "--save-seg", str(tmp_path / "seg"),
             "--seg-palette"])
    assert sorted(os.listdir(tmp_path / "seg")) == ["a.png", "b.png", "c.png"]
    mode, arr, table = png_map((tmp_path / "seg" / "b.png").read_bytes())
    assert mode == "P" and arr.shape == (270, 480) and table[3:6] == [128, 0, 128]


def test_save_seg_without_the_seg_head_raises(demo, tmp_path):
    from multitask_hydranet_amd import demo as DM
    from multitask_hydranet_amd import jpeg
    cfg = yaml.safe_load(open(TINY))
    cfg["train"]["train_seg"] = False
    path = tmp_path / "noseg.yml"
    path.write_text(yaml.safe_dump(cfg))
    write_jpegs(tmp_path / "images")
    with pytest.raises(ValueError):
        DM.main(["--cfg", str(path), "--images", str(tmp_path / "images"), "--out", str(tmp_path / "vis"), "--save-seg", str(tmp_path / "seg")])
    demo.train_seg = False
    try:
        with pytest.raises(ValueError):
            demo.process_device(jpeg.imread_bgr_device(avi_ref.clip()[1][0], device=demo.device), seg_png=True)
        with pytest.raises(ValueError):
            DM.run_images(demo, str(tmp_path / "images"), str(tmp_path / "vis2"), seg_dir=str(tmp_path / "seg2"))
    finally:
        demo.train_seg = True
