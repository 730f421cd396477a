"""GPU: the PNG label encode on the device (hn_png_enc.hip through multitask_hydranet_amd/png_encode.py) against the numpy restatement
(tests/png_enc_ref.py), stream for stream and record for record, into sentinel-filled buffers with a guard band around every stream slot
and around the workspace: the whole case matrix in ragged batches (int64 masks and packed uint8 maps), the capacity and range statuses
next to intact neighbours, the per-image host fallback, ragged batch against single calls, the resize against the float64 rule, and the
round trip through hn_png_decode.  Integer throughout: no tolerance."""
import io
import zlib

import numpy as np
import pytest
import torch
from PIL import Image

from multitask_hydranet_amd import png, png_encode
from multitask_hydranet_amd._lib import lib
from tests import png_enc_ref as R

pytestmark = pytest.mark.gpu

SENT = 0xA5
GUARD = 4096                            # bytes before / behind every stream slot and the workspace
DEV = "cuda:0"


def chunk():
    return int(lib().query("hn_png_enc_chunk_bytes"))


def encode_guarded(maps, out_sizes=None, caps=None, as_uint8=False):
    """hn_png_encode on one batch of class maps into sentinel-filled buffers -> (streams, status words).  Every stream slot has a guard
    band on both sides, so has the workspace, and the result array is longer than the batch.  Asserts the guards, that a refused image's
    slot is untouched, and that nothing lands at or past a slot's capacity."""
    n = len(maps)
    sizes = [tuple(m.shape) if out_sizes is None or out_sizes[i] is None else tuple(out_sizes[i]) for i, m in enumerate(maps)]
    raws = [h * (1 + w) for h, w in sizes]
    if caps is None:
        caps = [None] * n
    caps = [int(lib().query("hn_png_enc_cap_bytes", r)) if c is None else int(c) for r, c in zip(raws, caps)]
    max_raw, max_h = max(raws), max(h for h, _ in sizes)
    slot = (max_raw + 15) // 16 * 16
    desc = np.zeros(n, dtype=png_encode.DESC_DTYPE)
    soff, ooff = 0, GUARD
    for i, m in enumerate(maps):
        e = desc[i]
        e["src_off"], e["raw_off"], e["out_off"], e["out_cap"] = soff, i * slot, ooff, caps[i]
        e["Hs"], e["Ws"], e["Ho"], e["Wo"] = m.shape[0], m.shape[1], sizes[i][0], sizes[i][1]
        soff += m.size
        ooff += (caps[i] + 15) // 16 * 16 + GUARD
    flat = np.concatenate([np.asarray(m).reshape(-1) for m in maps])
    src = torch.from_numpy(flat.astype(np.uint8) if as_uint8 else flat.astype(np.int64)).to(DEV)
    out = torch.full((ooff,), SENT, dtype=torch.uint8, device=DEV)
    wsb = int(lib().query("hn_png_enc_ws_bytes", n, max_raw))
    assert wsb > 0
    ws = torch.full((GUARD + wsb + GUARD,), SENT, dtype=torch.uint8, device=DEV)
    result = torch.full((2 * (n + 4),), 77, dtype=torch.int64, device=DEV)
    desc_d = torch.from_numpy(desc.view(np.uint8).copy()).to(DEV)
    lib().call("hn_png_encode", src.data_ptr(), int(src.numel()), 0 if as_uint8 else 1, desc_d.data_ptr(), n, max_h, max_raw,
               ws.data_ptr() + GUARD, wsb, out.data_ptr(), ooff, result.data_ptr())
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    res = result.cpu().numpy()
    assert (res[2 * n:] == 77).all(), "the encode wrote past the result records"
    rec = res[:2 * n].view(png_encode.RESULT_DTYPE)
    assert (ws[:GUARD] == SENT).all().item() and (ws[GUARD + wsb:] == SENT).all().item(), "the encode wrote outside the workspace"
    streams, status, end = [], [], 0
    for i in range(n):
        o, cap, nb, st = int(desc[i]["out_off"]), caps[i], int(rec["stream_bytes"][i]), int(rec["status"][i])
        assert (host[end:o] == SENT).all(), "the encode wrote in front of stream slot %d" % i
        assert 0 <= nb <= cap
        if st != 0:
            assert nb == 0 and (host[o:o + cap] == SENT).all(), "a refused image's slot was written (%d)" % i
        used = (nb + 3) // 4 * 4
        assert (host[o + nb:o + used] == 0).all() and (host[o + used:o + (cap + 15) // 16 * 16] == SENT).all(), i
        streams.append(host[o:o + nb].tobytes())
        status.append(st)
        end = o + (cap + 15) // 16 * 16
    assert (host[end:] == SENT).all(), "the encode wrote behind the last stream slot"
    return streams, status


def pil_map(data):
    with Image.open(io.BytesIO(data)) as im:
        return im.mode, np.asarray(im).copy()


def test_matrix_streams_equal_the_restatement():
    """every case of the matrix, int64 masks, in four ragged batches (case k goes to batch k mod 4)"""
    rows, _ = R.encoded_cases(chunk())
    wrong = []
    for b in range(4):
        sel = rows[b::4]
        streams, status = encode_guarded([r[1] for r in sel], [r[2] for r in sel])
        for r, s, st in zip(sel, streams, status):
            if st != r[4] or s != r[3]:
                wrong.append((r[0], st, len(s), len(r[3])))
    assert not wrong, "device streams differ (case, status, bytes, expected bytes): %s" % wrong[:12]


def test_packed_uint8_maps_give_the_same_streams():
    rows, _ = R.encoded_cases(chunk())
    sel = [r for r in rows if r[1].size < 20000]
    assert len(sel) > 30
    streams, status = encode_guarded([r[1] for r in sel], [r[2] for r in sel], as_uint8=True)
    assert status == [0] * len(sel)
    assert [r[0] for r, s in zip(sel, streams) if s != r[3]] == []


def test_noise_default_capacity_then_half():
    """the 37 x 53 noise map is the worst case for size: the default capacity holds it; with half of it the image reports "full", writes
    nothing, and both neighbours are intact; encode_batch then hands that image to the host"""
    C = chunk()
    maps = [R.label_like(40, 64, 7), R.noise_map(), R.label_like(24, 40, 8)]
    want = [R.encode(m, None, C) for m in maps]
    streams, status = encode_guarded(maps)
    assert status == [0, 0, 0] and streams == [w[0] for w in want]
    assert len(want[1][0]) > maps[1].size                                 # noise does not compress with the fixed code
    half = int(lib().query("hn_png_enc_cap_bytes", 37 * 54)) // 2 // 4 * 4
    assert R.encode(maps[1], None, C, cap=half)[1] == R.ST_FULL
    streams, status = encode_guarded(maps, caps=[None, half, None])
    assert status == [0, png_encode.ST_FULL, 0]
    assert streams[0] == want[0][0] and streams[2] == want[2][0] and streams[1] == b""
    files = png_encode.encode_batch([m for m in maps], cap=[4096, half, 4096], device=DEV)
    for f, m in zip(files, maps):
        mode, arr = pil_map(f)
        assert mode == "L" and np.array_equal(arr, m)
    assert png.idat_bytes(png.parse(files[0])) == want[0][0] and png.idat_bytes(png.parse(files[2])) == want[2][0]
    assert png.idat_bytes(png.parse(files[1])) == png_encode.host_stream(maps[1])


def test_out_of_range_id_gets_the_range_status():
    C = chunk()
    good = R.label_like(24, 40, 8)
    bad = good.copy()
    bad[11, 17] = 256
    neg = good.copy()
    neg[0, 0] = -1
    streams, status = encode_guarded([good, bad, good, neg])
    assert status == [0, png_encode.ST_RANGE, 0, png_encode.ST_RANGE]
    want = R.encode(good, None, C)[0]
    assert streams == [want, b"", want, b""]
    assert R.encode(bad, None, C)[1] == R.ST_RANGE
    with pytest.raises(ValueError):
        png_encode.encode_batch([good, bad], device=DEV)


def test_bad_records_and_arguments_are_refused():
    good = R.label_like(24, 40, 8)
    streams, status = encode_guarded([good, good, good], caps=[None, 1022, None])      # a capacity that is no multiple of 4
    assert status == [0, png_encode.ST_RECORD, 0] and streams[0] == streams[2] != b""
    f = lib().raw("hn_png_encode")
    buf = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    p = buf.data_ptr()
    assert f(p, 16, 1, p, 0, 1, 16, p, 4096, p, 4096, p, None) == 1                      # N = 0
    assert f(p, 16, 1, p, 1, 1, 16, p, 16, p, 4096, p, None) == 1                        # a workspace that is too small
    assert f(p, 16, 2, p, 1, 1, 16, p, 4096, p, 4096, p, None) == 1                      # no such source type
    assert f(p, 16, 1, p, 1, 1, 1 << 30, p, 4096, p, 4096, p, None) == 1                 # raw size out of range
    torch.cuda.synchronize()


def test_ragged_batch_equals_single_calls_and_repeats():
    C = chunk()
    maps = [R.label_like(40, 64, 7), R.noise_map(), R.signed_noise(2 * C - 1, 3)[None], R.rows_repeat(256, 4), np.array([[9]], np.int64)]
    sizes = [(45, 77), None, None, None, (3, 5)]
    together, status = encode_guarded(maps, sizes)
    again, status2 = encode_guarded(maps, sizes)
    assert status == status2 == [0] * 5
    assert together == again
    for i, m in enumerate(maps):
        alone, st = encode_guarded([m], [sizes[i]])
        assert st == [0] and alone[0] == together[i], i


@pytest.mark.parametrize("src_hw,out_hw", [((24, 40), (45, 77)), ((24, 40), (24, 40)), ((17, 33), (1080, 1920))])
def test_resize_against_the_float64_rule(src_hw, out_hw):
    C = chunk()
    m = R.label_like(src_hw[0], src_hw[1], 21)
    stream, st, img, lines = R.encode(m, out_hw, C)
    got, status = encode_guarded([m], [out_hw])
    assert status == [0] and got[0] == stream
    assert zlib.decompress(got[0]) == lines.tobytes()
    mode, arr = pil_map(png_encode.assemble(out_hw[1], out_hw[0], got[0]))
    sx = np.minimum(np.floor(np.arange(out_hw[1]) * (1.0 / (out_hw[1] / src_hw[1]))).astype(np.int64), src_hw[1] - 1)
    sy = np.minimum(np.floor(np.arange(out_hw[0]) * (1.0 / (out_hw[0] / src_hw[0]))).astype(np.int64), src_hw[0] - 1)
    assert mode == "L" and np.array_equal(arr, m[np.ix_(sy, sx)])


def test_encode_batch_files_and_device_round_trip():
    """encode_batch on a device int64 mask [N, H, W] with one output size; hn_png_decode reads what hn_png_encode writes, grey and palette"""
    C = chunk()
    mask = torch.from_numpy(np.stack([R.label_like(24, 40, s) for s in (1, 2, 3)])).to(DEV)
    grey = png_encode.encode_batch(mask, out_sizes=(45, 77))
    pal = png_encode.encode_batch(mask, out_sizes=(45, 77), palette=R.PALETTE)
    for k in range(3):
        stream, st, img, lines = R.encode(mask[k].cpu().numpy(), (45, 77), C)
        assert grey[k] == R.assemble(77, 45, stream) and pal[k] == R.assemble(77, 45, stream, R.PALETTE)
        assert pil_map(grey[k])[0] == "L" and np.array_equal(pil_map(grey[k])[1], img)
        assert pil_map(pal[k])[0] == "P" and np.array_equal(pil_map(pal[k])[1], img)
    back = png.imread_label_device([grey[0], pal[1]], device=DEV)
    assert back["status"].cpu().tolist() == [0, 0]
    flat = back["data"].cpu().numpy()
    for j, k in enumerate((0, 1)):
        o = int(back["offsets"][j])
        assert tuple(back["shapes"][j]) == (45, 77)
        assert np.array_equal(flat[o:o + 45 * 77].reshape(45, 77), R.resize(mask[k].cpu().numpy(), (45, 77)))


def test_encode_batch_default_capacity_keeps_the_device_stream():
    """a size at which encode_batch's own capacity is the lean one (64 KB plus a quarter of the raw size, not the worst case): the file
    still carries the device's stream, not the host fallback's"""
    C = chunk()
    m = R.label_like(17, 33, 4)
    out_hw = (300, 401)
    raw = out_hw[0] * (1 + out_hw[1])
    assert (1 << 16) + raw // 4 < int(lib().query("hn_png_enc_cap_bytes", raw)) and ((1 << 16) + raw // 4) % 4 != 0
    stream, st, img, lines = R.encode(m, out_hw, C)
    files = png_encode.encode_batch([m], out_sizes=[out_hw], device=DEV)
    assert png.idat_bytes(png.parse(files[0])) == stream
    assert stream != png_encode.host_stream(m, out_hw)


def test_imwrite(tmp_path):
    m = R.label_like(24, 40, 5)
    path = tmp_path / "seg.png"
    png_encode.imwrite(str(path), m, device=DEV)
    with Image.open(str(path)) as im:
        assert im.mode == "L" and np.array_equal(np.asarray(im), m)
