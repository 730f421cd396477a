"""GPU: the JPEG scan decode on the device (hn_jpeg_scan.hip through multitask_hydranet_amd/jpeg.py) against the host's entropy stage,
element for element; the frames it leads to against PIL; MultitaskData(decode="device-entropy") -> HydraTrainer.to_gpu against
decode="host"; and the per-image fallback on a fixed list of eight damaged streams.  Integer throughout: no tolerance."""
import io

import numpy as np
import pytest
import torch

from multitask_hydranet_amd import dataset as D
from multitask_hydranet_amd import jpeg
from multitask_hydranet_amd._lib import lib
from tests import jpeg_cases as C
from tests import jpeg_scan_ref as SR
from tests.helpers import load_cfg

pytestmark = pytest.mark.gpu

SENT = 0x5A5A
GUARD = 4096                            # int16 entries behind the coefficients


def scan_decode_guarded(streams):
    """hn_jpeg_scan_decode on one batch of supported streams into a sentinel-filled buffer with a guard band behind it -> (per-image
    coefficients, status words)"""
    items = [jpeg.stream_stage(s) for s in streams]
    assert all(it[0] is not None for it in items)
    pk = jpeg.pack_streams(items)
    n, scans = len(items), pk["scans"]
    cb = int(pk["coef_bytes"])
    coefs = torch.full((cb // 2 + GUARD,), SENT, dtype=torch.int16, device="cuda:0")
    status = torch.full((n + 16,), 7, dtype=torch.int32, device="cuda:0")
    data = pk["data"].to("cuda:0")
    desc = torch.from_numpy(scans.view(np.uint8).copy()).to("cuda:0")
    max_scan, max_blocks = int(scans["scan_bytes"].max()), max(jpeg.n_blocks(it[0]) for it in items)
    wsb = int(lib().query("hn_jpeg_scan_ws_bytes", n, max_scan, max_blocks))
    ws = torch.empty((wsb,), dtype=torch.uint8, device="cuda:0")
    lib().call("hn_jpeg_scan_decode", data.data_ptr(), int(data.numel()), desc.data_ptr(), n, max_scan, max_blocks, ws.data_ptr(), wsb,
               coefs.data_ptr(), cb, status.data_ptr())
    torch.cuda.synchronize()
    flat, st = coefs.cpu().numpy(), status.cpu().numpy()
    assert (flat[cb // 2:] == SENT).all(), "the scan decode wrote past the coefficient buffer"
    assert (st[n:] == 7).all(), "the scan decode wrote past the status words"
    out = [flat[int(r["coef_off"]) // 2:int(r["coef_off"]) // 2 + it[0]["coef_bytes"] // 2].reshape(-1, 64) for r, it in zip(scans, items)]
    return out, st[:n]


def test_full_matrix_coefficients_equal_the_host_entropy_stage():
    """all 216 streams of the matrix and the three committed frames, in ragged batches that mix sub-samplings, sizes from 1x1 to 1570x660
    and restart intervals (stream k goes to batch k mod 8): coefficients equal jpeg.entropy_decode's element for element, status 0"""
    streams = [C.encode(case) for case in C.MATRIX] + [C.golden_bytes(n) for n in C.GOLDEN_FRAMES]
    names = [C.case_id(case) for case in C.MATRIX] + list(C.GOLDEN_FRAMES)
    assert len(streams) == 219
    wrong, checked = [], 0
    for b in range(8):
        sel = list(range(b, len(streams), 8))
        got, st = scan_decode_guarded([streams[k] for k in sel])
        for k, g, s in zip(sel, got, st):
            want = jpeg.entropy_decode(streams[k], jpeg.parse(streams[k]))
            checked += 1
            if s != 0 or g.shape != want.shape or not np.array_equal(g, want):
                wrong.append((names[k], int(s), int((g != want).sum()) if g.shape == want.shape else -1))
    assert checked == 219
    assert not wrong, "device coefficients differ (name, status, entries off): %s" % wrong[:12]


def _progressive():
    from PIL import Image
    bio = io.BytesIO()
    Image.fromarray(C.seeded_image(96, 64, 3)).save(bio, "JPEG", quality=80, progressive=True)
    return bio.getvalue()


def test_frames_equal_coefficient_path_and_pil():
    cases = [c for c in C.MATRIX if c[3] in ((1, 1), (17, 33), (157, 66)) and c[1] == 75] + [("4:2:0", 95, True, (640, 360), 4)]
    streams = [C.encode(c) for c in cases] + [C.golden_bytes("frame_1570x660.jpg")]
    streams.insert(3, _progressive())
    a = jpeg.decode_batch(jpeg.pack_streams([jpeg.stream_stage(s) for s in streams]), device="cuda:0")
    b = jpeg.decode_batch(jpeg.pack_coefs([jpeg.host_stage(s) for s in streams]), device="cuda:0")
    torch.cuda.synchronize()
    assert jpeg.stream_stage(streams[3])[0] is None
    assert np.array_equal(a["offsets"], b["offsets"]) and np.array_equal(a["shapes"], b["shapes"]) and torch.equal(a["data"], b["data"])
    flat = a["data"].cpu().numpy()
    for i, s in enumerate(streams):
        h, w = (int(v) for v in a["shapes"][i])
        assert np.array_equal(flat[a["offsets"][i]:a["offsets"][i] + h * w * 3].reshape(h, w, 3), C.pil_bgr(s)), i
    one = jpeg.imread_bgr_device(streams[-1], device="cuda:0", entropy="device")
    assert one["shapes"].tolist() == [[660, 1570]] and np.array_equal(one["data"].cpu().numpy().reshape(660, 1570, 3), C.pil_bgr(streams[-1]))


def test_trainer_device_entropy_decode_equals_host_decode(tmp_path):
    """as test_jpeg_gpu.py's check of decode="device": the batch to_gpu makes from decode="device-entropy" equals the decode="host" one"""
    from multitask_hydranet_amd.train import HydraTrainer
    cfgs = load_cfg("hydranet_tiny.yml")
    dl = cfgs["dataloader"]
    tree = C.write_tree(str(tmp_path), [(n, C.golden_bytes(n)) for n in C.GOLDEN_FRAMES], (dl["network_input_height"], dl["network_input_width"]))
    dl.update(tree["dataloader"])
    torch.manual_seed(0)
    tr = HydraTrainer(cfgs, iters_per_epoch=10)
    got = {}
    for mode in ("host", "device-entropy"):
        ds = D.MultitaskData(cfgs, "train", base_seed=4, decode=mode)
        ds.set_epoch(3)
        batch = ds.collate_fn([ds[i] for i in range(len(ds))])
        assert ("src_streams" in batch) == (mode == "device-entropy") and ("src_frames" in batch) == (mode == "host")
        got[mode] = tr.to_gpu(batch)
    torch.cuda.synchronize()
    assert any(p["augmented"] and (p["photo"] or p["geom"]) for p in batch["aug_plans"])
    for k in ("image", "gt_seg", "gt_det", "gt_cls", "gt_loc"):
        a, b = got["host"][k], got["device-entropy"][k]
        assert a.is_cuda and b.is_cuda and a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b), k
    assert got["host"]["annot_lane"] == got["device-entropy"]["annot_lane"]
    assert "src_streams" not in got["device-entropy"] and "src_frames" not in got["device-entropy"]


def damaged_streams():
    """the fixed list: three truncations inside the scan and five seeded single-byte changes of one 157x66 restart-interval stream"""
    base = C.encode(("4:2:0", 75, False, (157, 66), 4))
    scan = int(jpeg.parse(base)["scan_offset"])
    out = [base[:scan + 10], base[:(scan + len(base)) // 2], base[:len(base) - 5]]
    for seed in range(5):
        rng = np.random.default_rng(seed)
        b = bytearray(base)
        b[int(rng.integers(scan, len(base) - 2))] = int(rng.integers(0, 256))
        out.append(bytes(b))
    return base, out


def test_damaged_streams_stay_in_bounds_and_fall_back_to_pil():
    base, bad = damaged_streams()
    assert len(bad) == 8
    S = int(lib().query("hn_jpeg_scan_subseq_bytes"))
    want_status = []
    for s in bad:
        head = jpeg.parse(s)
        SR.decode(s, head, jpeg.scan_prepare(s, head), S)              # the restatement asserts every index it forms
        want_status.append(jpeg.entropy_status(s, head, np.empty((jpeg.n_blocks(head), 64), dtype=np.int16)))
    _, st = scan_decode_guarded([base] + bad)                            # asserts the guard band
    assert st[0] == 0 and set(st.tolist()) <= {0, 1}
    assert st[1:].tolist() == want_status, (st[1:].tolist(), want_status)
    assert 0 in want_status and 1 in want_status
    pils = []
    for s in bad:
        try:
            pils.append(C.pil_bgr(s))
        except Exception:
            pils.append(None)
    keep = [i for i, p in enumerate(pils) if p is not None]
    assert any(want_status[i] == 1 for i in keep)
    out = jpeg.decode_batch(jpeg.pack_streams([jpeg.stream_stage(bad[i]) for i in keep]), device="cuda:0")
    flat = out["data"].cpu().numpy()
    for k, i in enumerate(keep):
        if want_status[i] == 1:
            assert np.array_equal(flat[out["offsets"][k]:out["offsets"][k] + pils[i].size].reshape(pils[i].shape), pils[i]), i
    gone = [i for i, p in enumerate(pils) if p is None]
    if gone:                                                             # a file PIL cannot decode either raises, as in the other modes
        with pytest.raises(Exception):
            jpeg.decode_batch(jpeg.pack_streams([jpeg.stream_stage(bad[gone[0]])]), device="cuda:0")
