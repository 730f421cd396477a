"""GPU: the device half of the JPEG decode (hn_jpeg.hip through multitask_hydranet_amd/jpeg.py) against PIL and against the integer
restatement tests/jpeg_ref.py, exactly; and through MultitaskData(decode="device") -> HydraTrainer.to_gpu against decode="host"."""
import numpy as np
import pytest
import torch

from multitask_hydranet_amd import dataset as D
from multitask_hydranet_amd import jpeg
from tests import jpeg_cases as C
from tests import jpeg_ref as R
from tests.helpers import load_cfg

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5


def test_ragged_batch_equals_pil_and_restatement():
    """one ragged batch: the whole matrix of tests/test_jpeg_cpu.py, the committed frames and one frame decoded elsewhere; the output
    buffer is pre-filled with a sentinel (pixels the kernels leave unwritten show as 0xA5 runs)"""
    streams = [C.encode(case) for case in C.MATRIX] + [C.golden_bytes(n) for n in C.GOLDEN_FRAMES]
    names = [C.case_id(case) for case in C.MATRIX] + list(C.GOLDEN_FRAMES)
    items = [jpeg.host_stage(s) for s in streams]
    assert all(h is not None for h, _ in items)
    straggler = C.seeded_image(37, 21, 1)
    items.insert(5, (None, straggler))
    total = sum(int(np.prod(C.pil_bgr(s).shape)) for s in streams) + straggler.size
    buf = torch.full((total + 4096,), SENTINEL, dtype=torch.uint8, device="cuda:0")
    out = jpeg.decode_batch(items, device="cuda:0", out=buf)
    torch.cuda.synchronize()
    assert out["data"].is_cuda and out["data"].dtype == torch.uint8
    flat = out["data"].cpu().numpy()
    offs, shapes = out["offsets"], out["shapes"]
    assert out["data"].data_ptr() == buf.data_ptr() and int(offs[-1] + shapes[-1, 0] * shapes[-1, 1] * 3) == total
    assert (flat[total:] == SENTINEL).all(), "written past the last frame"
    got5 = flat[offs[5]:offs[5] + straggler.size].reshape(straggler.shape)
    assert np.array_equal(got5, straggler)
    wrong = []
    for k, ((head, coefs), data, name) in enumerate(zip(items[:5] + items[6:], streams, names)):
        i = k if k < 5 else k + 1
        h, w = int(shapes[i, 0]), int(shapes[i, 1])
        got = flat[offs[i]:offs[i] + h * w * 3].reshape(h, w, 3)
        pil, ref = C.pil_bgr(data), R.decode(head, coefs)
        assert got.shape == pil.shape, name
        if not np.array_equal(got, pil) or not np.array_equal(got, ref):
            wrong.append((name, int(np.abs(got.astype(int) - pil).max()), int(np.abs(got.astype(int) - ref).max()), int((got != pil).sum())))
    assert not wrong, "device frames differ (name, max |got - PIL|, max |got - restatement|, bytes off PIL): %s" % wrong[:10]


def test_imread_bgr_device_one_call():
    data = C.golden_bytes("frame_1570x660.jpg")
    out = jpeg.imread_bgr_device(data, device="cuda:0")
    assert out["shapes"].tolist() == [[660, 1570]] and np.array_equal(out["data"].cpu().numpy().reshape(660, 1570, 3), C.pil_bgr(data))


def test_trainer_device_decode_equals_host_decode(tmp_path):
    """a data list over the committed frames with synthetic lane / box / label files, augmentation on: for the same (base_seed, epoch,
    index) the batch to_gpu makes from decode="device" equals the one from decode="host" bit for bit"""
    from multitask_hydranet_amd.train import HydraTrainer
    cfgs = load_cfg("hydranet_tiny.yml")
    dl = cfgs["dataloader"]
    tree = C.write_tree(str(tmp_path), [(n, C.golden_bytes(n)) for n in C.GOLDEN_FRAMES], (dl["network_input_height"], dl["network_input_width"]))
    dl.update(tree["dataloader"])
    torch.manual_seed(0)
    tr = HydraTrainer(cfgs, iters_per_epoch=10)
    got = {}
    for mode in ("host", "device"):
        ds = D.MultitaskData(cfgs, "train", base_seed=4, decode=mode)
        ds.set_epoch(3)
        batch = ds.collate_fn([ds[i] for i in range(len(ds))])
        assert ("src_coefs" in batch) == (mode == "device") and ("src_frames" in batch) == (mode == "host")
        got[mode] = tr.to_gpu(batch)
    torch.cuda.synchronize()
    assert any(p["augmented"] and (p["photo"] or p["geom"]) for p in batch["aug_plans"])
    for k in ("image", "gt_seg", "gt_det", "gt_cls", "gt_loc"):
        a, b = got["host"][k], got["device"][k]
        assert a.is_cuda and b.is_cuda and a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b), k
    assert got["host"]["annot_lane"] == got["device"]["annot_lane"]
    assert "src_coefs" not in got["device"] and "src_frames" not in got["device"]
