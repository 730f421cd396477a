"""GPU: the demo's seg class maps as label PNGs with the dynamic-Huffman deflate (--save-seg with --seg-huffman dynamic; Demo.process_device /
process_device_batch with seg_huffman="dynamic"): the files decode to the maps the fixed-code run writes, none is larger than its
fixed-code counterpart, and the option is refused without --save-seg.  Tiny cfg, recorded weights."""
import io
import os

import numpy as np
import pytest
from PIL import Image

from tests import avi_ref
from tests.test_demo_images_gpu import make_demo
from tests.test_demo_seg_png_gpu import TINY, write_jpegs

pytestmark = pytest.mark.gpu


def png_map(data):
    with Image.open(io.BytesIO(data)) as im:
        return im.mode, np.asarray(im).copy()


def test_command_line_seg_huffman_dynamic(tmp_path):
    from multitask_hydranet_amd import demo as DM
    write_jpegs(tmp_path / "images")
    common = ["--cfg", TINY, "--images", str(tmp_path / "images")]
    DM.main(common + ["--out", str(tmp_path / "vis_f"), "--save-seg", str(tmp_path / "seg_f")])
    DM.main(common + ["--out", str(tmp_path / "vis_d"), "--save-seg", str(tmp_path / "seg_d"), "--seg-huffman", "dynamic"])
    assert sorted(os.listdir(tmp_path / "seg_d")) == ["a.png", "b.png", "c.png"] == sorted(os.listdir(tmp_path / "seg_f"))
    for jpg in ("a.jpg", "b.jpg", "c.jpeg"):
        name = os.path.splitext(jpg)[0] + ".png"
        fixed, dyn = (tmp_path / "seg_f" / name).read_bytes(), (tmp_path / "seg_d" / name).read_bytes()
        (mode_f, arr_f), (mode_d, arr_d) = png_map(fixed), png_map(dyn)
        print(name, "fixed %d B, dynamic %d B" % (len(fixed), len(dyn)))
        assert mode_f == mode_d == "L" and np.array_equal(arr_f, arr_d), name
        assert len(dyn) <= len(fixed), (name, len(dyn), len(fixed))
        assert (tmp_path / "vis_d" / jpg).read_bytes() == (tmp_path / "vis_f" / jpg).read_bytes(), jpg
    with pytest.raises(SystemExit):
        DM.main(common + ["--out", str(tmp_path / "vis_x"), "--seg-huffman", "dynamic"])


def test_process_device_and_batch_seg_huffman():
    from multitask_hydranet_amd import jpeg
    demo = make_demo()
    clip = list(avi_ref.clip()[1][:2])
    fixed = demo.process_device_batch(jpeg.imread_bgr_device(clip, device=demo.device), seg_png=True)
    dyn = demo.process_device_batch(jpeg.imread_bgr_device(clip, device=demo.device), seg_png=True, seg_huffman="dynamic")
    assert dyn["jpeg"] == fixed["jpeg"] and len(dyn["seg_png"]) == 2
    for k in range(2):
        assert np.array_equal(png_map(dyn["seg_png"][k])[1], png_map(fixed["seg_png"][k])[1]), k
        assert len(dyn["seg_png"][k]) <= len(fixed["seg_png"][k]), k
        alone = demo.process_device(jpeg.imread_bgr_device(clip[k], device=demo.device), seg_png=True, seg_huffman="dynamic")
        assert alone["seg_png"] == dyn["seg_png"][k], k
    with pytest.raises(ValueError):
        demo.process_device(jpeg.imread_bgr_device(clip[0], device=demo.device), seg_png=True, seg_huffman="bogus")
