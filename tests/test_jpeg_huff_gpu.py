"""GPU: the JPEG encode's entropy stage on the device (hn_jpeg_huff.hip through multitask_hydranet_amd/jpeg_encode.py) against the host
stage hn_jpeg_entropy_encode, byte for byte, with the output buffer and the workspace's tail sentinel-filled.  Exact."""
import numpy as np
import pytest
import torch

from multitask_hydranet_amd import jpeg, jpeg_encode as JE
from multitask_hydranet_amd._lib import lib
from tests import jpeg_cases as C
from tests import jpeg_enc_ref as E
from tests.test_jpeg_encode_cpu import GOLDEN_FRAMES, MATRIX, SUBSAMPLINGS, case_id, case_image, golden_bgr, pil_encode
from tests.test_jpeg_huff_cpu import HAND

pytestmark = pytest.mark.gpu

SENT = 0xC3
GAP = 37                               # sentinel bytes between two images' ranges of the output buffer (odd: unaligned ranges)
TAIL = 4096                            # sentinel bytes behind the workspace


def raw_encode(heads, cos, caps, ws=None):
    """the raw call on coefficient arrays uploaded as they are -> (status, scan_bytes, scans, ws).  Every byte of `out` outside the
    written scans, and the workspace's tail, must still hold the sentinel."""
    n = len(heads)
    coff = np.zeros(n + 1, np.int64)
    for i, h in enumerate(heads):
        coff[i + 1] = coff[i] + (h["coef_bytes"] + 15) // 16 * 16
    flat = np.full(int(coff[-1]) // 2, 0x7B7B, np.int16)
    for i, co in enumerate(cos):
        flat[int(coff[i]) // 2:int(coff[i]) // 2 + co.size] = np.asarray(co, np.int16).reshape(-1)
    coefs = torch.from_numpy(flat).to("cuda:0")
    desc, ooff = JE.huff_describe(heads, coff, [c + GAP for c in caps])
    desc["out_cap"] = caps
    desc["out_off"] += GAP
    max_blocks, max_cap = max(h["coef_bytes"] // 128 for h in heads), max(caps)
    need = JE.huff_workspace_bytes(n, max_blocks, max_cap)
    if ws is None:
        ws = torch.full((need + TAIL,), SENT, dtype=torch.uint8, device="cuda:0")
    assert ws.numel() >= need + TAIL
    ws[need:] = SENT
    out = torch.full((int(ooff[-1]) + GAP,), SENT, dtype=torch.uint8, device="cuda:0")
    res = torch.full((n * 16,), SENT, dtype=torch.uint8, device="cuda:0")
    desc_d = torch.from_numpy(desc.view(np.uint8).copy()).to("cuda:0")
    lib().call("hn_jpeg_huff_encode", coefs.data_ptr(), int(coefs.numel()) * 2, desc_d.data_ptr(), n, max_blocks, max_cap, ws.data_ptr(), need,
               out.data_ptr(), int(out.numel()), res.data_ptr())
    torch.cuda.synchronize()
    assert bool((ws[need:] == SENT).all()), "written past the workspace"
    r = res.cpu().numpy().view(JE.HUFF_RESULT_DTYPE)
    o = out.cpu().numpy()
    status, nbytes, scans, pos = r["status"].tolist(), r["scan_bytes"].tolist(), [], 0
    for i in range(n):
        a = int(desc["out_off"][i])
        assert (o[pos:a] == SENT).all(), "written between two images (before image %d)" % i
        assert 0 <= nbytes[i] <= caps[i] and (status[i] == 0 or nbytes[i] == 0), (i, status[i], nbytes[i], caps[i])
        scans.append(o[a:a + nbytes[i]].tobytes())
        pos = a + nbytes[i]                                              # behind the scan: sentinel up to the next image, capacity included
    assert (o[pos:] == SENT).all(), "written behind the last image"
    return status, nbytes, scans, ws


def host_streams(heads, cos):
    return [JE.entropy_encode(np.asarray(co, np.int16), h) for h, co in zip(heads, cos)]


def compare(heads, cos, names, ws=None):
    host = host_streams(heads, cos)
    hdr = [JE.write_header(h) for h in heads]
    caps = [len(s) - len(x) - 2 + (i % 3) * 5 for i, (s, x) in enumerate(zip(host, hdr))]      # exact, and a little more
    status, nbytes, scans, ws = raw_encode(heads, cos, caps, ws)
    wrong = []
    for i, name in enumerate(names):
        want = host[i][len(hdr[i]):-2]
        same = status[i] == 0 and scans[i] == want
        print("device vs host: %s status %d scan bytes %d host %d equal %s" % (name, status[i], nbytes[i], len(want), same))
        if not same:
            wrong.append((name, status[i], nbytes[i], len(want)))
    assert not wrong, "device scans differ (name, status, bytes, host bytes): %s" % wrong[:10]
    return ws


def matrix_inputs(cases):
    heads = [JE.make_head(c[2][0], c[2][1], c[1], c[0]) for c in cases]
    return heads, [E.encode_coefs(case_image(c), c[0], c[1])[1] for c in cases], [case_id(c) for c in cases]


def test_matrix_as_one_ragged_batch_equals_host():
    compare(*matrix_inputs(MATRIX))


@pytest.mark.parametrize("ss", SUBSAMPLINGS)
def test_committed_frames_equal_host(ss):
    frames = [golden_bgr(n) for n in GOLDEN_FRAMES]                      # the first is 2560 x 1440: several tiles at every scan level
    heads = [JE.make_head(f.shape[1], f.shape[0], 95, ss) for f in frames]
    compare(heads, [E.encode_coefs(f, ss, 95)[1] for f in frames], ["%s-%s" % (ss, n) for n in GOLDEN_FRAMES])


def test_hand_made_coefficients_equal_host():
    compare([JE.make_head(w, h, 95, ss) for _, w, h, ss, _ in HAND], [c[4] for c in HAND], [c[0] for c in HAND])


def test_two_calls_on_one_workspace():
    """the workspace is not cleared between calls: a large batch, then a different, smaller one over its leftovers, then the first again"""
    a = matrix_inputs([c for c in MATRIX if c[2] in ((157, 66), (640, 360))])
    b = ([JE.make_head(w, h, 95, ss) for _, w, h, ss, _ in HAND[:12]], [c[4] for c in HAND[:12]], [c[0] for c in HAND[:12]])
    ws = compare(*a)
    compare(*b, ws=ws)
    compare(*a, ws=ws)


def test_undersized_capacity_is_reported_and_nothing_is_written():
    cases = [("4:2:0", 95, (157, 66)), ("grey", 75, (17, 33)), ("4:2:2", 95, (640, 360))]
    heads, cos, names = matrix_inputs(cases)
    full = [len(s) - len(JE.write_header(h)) - 2 for s, h in zip(host_streams(heads, cos), heads)]
    for cut in (1, 2, 100, 10 ** 9):
        caps = [max(0, full[0] - cut), full[1], max(0, full[2] - cut)]
        status, nbytes, scans, _ = raw_encode(heads, cos, caps)        # (raw_encode checks that every byte outside the scans is untouched)
        assert status == [JE.CAPACITY_TOO_SMALL, 0, JE.CAPACITY_TOO_SMALL] and nbytes == [0, full[1], 0], (cut, status, nbytes)
        assert scans[1] == host_streams(heads[1:2], cos[1:2])[0][-2 - full[1]:-2]


def test_encode_batch_grows_a_small_first_capacity(monkeypatch):
    cases = [c for c in MATRIX if c[1] == 95 and c[0] == "4:2:0"]
    frames = [case_image(c) for c in cases]
    want = JE.encode_batch(frames, 95, "4:2:0")
    monkeypatch.setattr(JE, "first_capacity", lambda head: 16)
    assert JE.encode_batch(frames, 95, "4:2:0", entropy="device") == want
    monkeypatch.undo()
    assert JE.encode_batch(frames, 95, "4:2:0", entropy="device") == want


def test_one_image_out_of_range_in_a_batch():
    heads = [JE.make_head(24, 24, 75, ss) for ss in ("4:2:0", "4:2:0", "grey", "4:4:4")]
    cos = [np.zeros((h["coef_bytes"] // 128, 64), np.int16) for h in heads]
    for co in cos:
        co[:, 0], co[:, 9] = 1023, -1023
    host = host_streams(heads, cos)
    caps = [len(s) for s in host]
    for b, k, v in ((1, 5, 1024), (2, 63, -1024), (1, 0, -1025), (0, 0, 2048)):
        bad = [c.copy() for c in cos]
        bad[1][b, k] = v
        assert JE.entropy_status(bad[1], heads[1], np.empty(1 << 16, np.uint8)) == -1
        status, nbytes, scans, _ = raw_encode(heads, bad, caps)
        assert status == [0, -1, 0, 0] and nbytes[1] == 0, (b, k, v, status, nbytes)
        for i in (0, 2, 3):
            assert scans[i] == host[i][len(JE.write_header(heads[i])):-2]
        coff = np.zeros(5, np.int64)
        coff[1:] = np.cumsum([h["coef_bytes"] for h in heads])
        dev = torch.from_numpy(np.concatenate([c.reshape(-1) for c in bad])).to("cuda:0")
        with pytest.raises(ValueError, match="image 1"):
            JE.entropy_encode_device(heads, dev, coff)
    good = torch.from_numpy(np.concatenate([c.reshape(-1) for c in cos])).to("cuda:0")
    assert JE.entropy_encode_device(heads, good, coff) == host


def test_encode_batch_device_equals_host_and_pil_decodes_it():
    for ss in SUBSAMPLINGS:
        for q in (75, 95):
            sel = [c for c in MATRIX if c[0] == ss and c[1] == q]
            frames = [case_image(c) for c in sel]
            blobs = JE.encode_batch(frames, q, ss, entropy="device")
            assert blobs == JE.encode_batch(frames, q, ss) == JE.encode_batch(frames, q, ss, entropy="host")
            for c, f, b in zip(sel, frames, blobs):
                want = C.pil_bgr(pil_encode(f, ss, q))
                got = C.pil_bgr(b)
                assert got.shape == want.shape and np.array_equal(got, want), case_id(c)
    with pytest.raises(ValueError):
        JE.encode_batch(frames, 95, "4:2:0", entropy="Device")


def test_imwrite_device(tmp_path):
    f = golden_bgr(GOLDEN_FRAMES[1])
    JE.imwrite(str(tmp_path / "h.jpg"), f, quality=75, subsampling="4:2:2")
    JE.imwrite(str(tmp_path / "d.jpg"), f, quality=75, subsampling="4:2:2", entropy="device")
    assert open(str(tmp_path / "h.jpg"), "rb").read() == open(str(tmp_path / "d.jpg"), "rb").read()


def test_run_images_writes_identical_files(tmp_path):
    """the demo over a folder, tiny model with recorded weights (thresholds that let it draw lanes and boxes)"""
    from multitask_hydranet_amd.demo import Demo, run_images
    from tests.helpers import load_cfg, load_npz, tiny_state
    src = tmp_path / "in"
    src.mkdir()
    for name in GOLDEN_FRAMES:
        (src / name).write_bytes(C.golden_bytes(name))
    demo = Demo(load_cfg("hydranet_tiny.yml"), fold_batchnorm=False)
    demo.net.load_state_dict(tiny_state(load_npz("tiny_hydranet.npz")))
    demo.net.eval().prepare_inference()
    demo.lane_conf, demo.det_conf = 0.3, 0.3
    run_images(demo, str(src), str(tmp_path / "host"), entropy="host")
    run_images(demo, str(src), str(tmp_path / "device"), entropy="device")
    for name in GOLDEN_FRAMES:
        a, b = (tmp_path / "host" / name).read_bytes(), (tmp_path / "device" / name).read_bytes()
        assert len(a) > 1000 and a == b, name
