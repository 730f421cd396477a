"""GPU: the device half of the JPEG encode (hn_jpeg_enc.hip through multitask_hydranet_amd/jpeg_encode.py) against the integer restatement
tests/jpeg_enc_ref.py, coefficient for coefficient, and the streams of encode_batch against PIL's own encoder, pixel for pixel.  Exact."""
import numpy as np
import pytest
import torch

from multitask_hydranet_amd import jpeg, jpeg_encode as JE
from multitask_hydranet_amd.augment import pack
from tests import jpeg_cases as C
from tests import jpeg_enc_ref as E
from tests.test_jpeg_encode_cpu import GOLDEN_FRAMES, MATRIX, SUBSAMPLINGS, case_id, case_image, golden_bgr, pil_encode

pytestmark = pytest.mark.gpu

SENTINEL = 0x7B7B


def device_pack(frames, lead=21):
    """the frames packed on the device behind `lead` stray bytes, so that no frame starts on an aligned address"""
    pk = pack([np.full((1, lead // 3, 3), 9, np.uint8)] + list(frames))
    return {"data": pk["data"].to("cuda:0"), "offsets": pk["offsets"][1:], "shapes": pk["shapes"][1:]}


def device_coefs(frames, quality, subsampling):
    """-> (heads, list of int16 [blocks, 64] per image); the output buffer is sentinel-filled and checked outside the images' ranges"""
    n = len(frames)
    subs = [subsampling] * n if isinstance(subsampling, str) else subsampling
    quals = [quality] * n if np.isscalar(quality) else quality
    need = sum((JE.make_head(f.shape[1], f.shape[0], q, s)["coef_bytes"] + 15) // 16 * 16 for f, q, s in zip(frames, quals, subs))
    buf = torch.full((need // 2 + 2048,), SENTINEL, dtype=torch.int16, device="cuda:0")
    heads, coefs, coff = JE.encode_coefs_device(device_pack(frames), quals, subs, out=buf)
    torch.cuda.synchronize()
    assert coefs.data_ptr() == buf.data_ptr() and int(coff[-1]) == need
    flat = coefs.cpu().numpy()
    assert (flat[need // 2:] == SENTINEL).all(), "written past the last image"
    out = []
    for i, h in enumerate(heads):
        a, b = int(coff[i]) // 2, int(coff[i]) // 2 + h["coef_bytes"] // 2
        out.append(flat[a:b].reshape(-1, 64))
        assert (flat[b:int(coff[i + 1]) // 2] == SENTINEL).all(), "written between two images"
    return heads, out


def compare(frames, quals, subs, names):
    heads, got = device_coefs(frames, quals, subs)
    wrong = []
    for f, q, s, name, h, g in zip(frames, quals, subs, names, heads, got):
        rh, ref = E.encode_coefs(f, s, q)
        assert g.shape == ref.shape and h["coef_bytes"] == rh["coef_bytes"], name
        bad = int((g != ref).any(axis=1).sum())
        print("device vs restatement: %s blocks %d differing %d unwritten %d" % (name, ref.shape[0], bad, int((g == SENTINEL).all(axis=1).sum())))
        if bad:
            wrong.append((name, bad, int(np.abs(g.astype(int) - ref).max())))
    assert not wrong, "device coefficients differ (name, blocks, max |difference|): %s" % wrong[:10]


def test_matrix_equals_restatement():
    """sub-sampling x quality x size, one image per launch would hide nothing a ragged launch shows: all in one batch"""
    frames = [case_image(c) for c in MATRIX]
    compare(frames, [c[1] for c in MATRIX], [c[0] for c in MATRIX], [case_id(c) for c in MATRIX])


@pytest.mark.parametrize("case", [c for c in MATRIX if c[2] in ((1, 1), (17, 33), (157, 66))], ids=case_id)
def test_single_image_equals_restatement(case):
    compare([case_image(case)], [case[1]], [case[0]], [case_id(case)])


@pytest.mark.parametrize("ss", SUBSAMPLINGS)
def test_committed_frames_equal_restatement(ss):
    compare([golden_bgr(n) for n in GOLDEN_FRAMES], [95, 75, 95], [ss] * 3, list(GOLDEN_FRAMES))


def test_wide_frame_crosses_strip_boundaries():
    """widths around the 512-pixel strip of the kernel, odd heights"""
    sizes = ((511, 9), (512, 16), (513, 17), (1025, 31), (1536, 15))
    frames = [np.ascontiguousarray(C.seeded_image(w, h, 40 + w)[..., ::-1]) for w, h in sizes]
    for ss in SUBSAMPLINGS:
        compare(frames, [90] * len(frames), [ss] * len(frames), ["%s-%dx%d" % ((ss,) + s) for s in sizes])


def test_encode_batch_decodes_to_what_pils_encode_decodes_to():
    cases = [c for c in MATRIX if c[1] in (75, 95)]
    for ss in SUBSAMPLINGS:
        for q in (75, 95):
            sel = [c for c in cases if c[0] == ss and c[1] == q]
            frames = [case_image(c) for c in sel]
            blobs = JE.encode_batch(frames, q, ss)                       # a list of host arrays: uploaded
            assert len(blobs) == len(frames)
            for c, f, b in zip(sel, frames, blobs):
                want = C.pil_bgr(pil_encode(f, ss, q))
                got = C.pil_bgr(b)
                assert got.shape == want.shape and np.array_equal(got, want), case_id(c)


def test_round_trip_equals_pils(tmp_path):
    """decode -> encode -> decode through jpeg.imread_bgr_device and encode_batch equals the same trip through PIL, on the committed frames"""
    for name in GOLDEN_FRAMES:
        data = C.golden_bytes(name)
        frames = jpeg.imread_bgr_device(data, device="cuda:0")
        blob = JE.encode_batch(frames, 95, "4:2:0")[0]
        want = C.pil_bgr(pil_encode(C.pil_bgr(data), "4:2:0", 95))
        back = jpeg.imread_bgr_device(blob, device="cuda:0")
        h, w = want.shape[:2]
        assert back["shapes"].tolist() == [[h, w]]
        assert np.array_equal(back["data"].cpu().numpy()[:h * w * 3].reshape(h, w, 3), want), name
        assert np.array_equal(C.pil_bgr(blob), want), name
    p = str(tmp_path / "one.jpg")
    JE.imwrite(p, golden_bgr(GOLDEN_FRAMES[1]), quality=75, subsampling="4:2:2")
    with open(p, "rb") as f:
        assert np.array_equal(C.pil_bgr(f.read()), C.pil_bgr(pil_encode(golden_bgr(GOLDEN_FRAMES[1]), "4:2:2", 75)))


def test_descriptor_that_does_not_fit_is_left_unwritten():
    """the kernel checks every descriptor against the buffer sizes: with the byte counts cut short nothing is written"""
    from multitask_hydranet_amd._lib import lib
    f = case_image(("4:2:0", 75, (157, 66)))
    pk = device_pack([f])
    heads, desc, coff = JE.describe_batch(pk["shapes"], pk["offsets"], 75, "4:2:0")
    desc_d = torch.from_numpy(desc.view(np.uint8).copy()).to("cuda:0")
    for frames_bytes, coef_bytes in ((int(pk["data"].numel()) - 1, int(coff[-1])), (int(pk["data"].numel()), int(coff[-1]) - 16)):
        buf = torch.full((int(coff[-1]) // 2 + 64,), SENTINEL, dtype=torch.int16, device="cuda:0")
        lib().call("hn_jpeg_encode", pk["data"].data_ptr(), frames_bytes, desc_d.data_ptr(), 1, heads[0]["mcus_y"], heads[0]["mcus_x"] * 16, buf.data_ptr(),
                   coef_bytes)
        torch.cuda.synchronize()
        assert bool((buf == SENTINEL).all())
