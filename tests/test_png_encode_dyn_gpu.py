"""GPU: the PNG label encode with dynamic-Huffman blocks (hn_png_encode_dyn in hn_png_enc.hip, png_encode's huffman="dynamic") against its
restatement (tests/png_enc_dyn_ref.py), stream for stream and record for record, by test_png_encode_gpu.py's method: sentinel-filled
buffers with a guard band around every stream slot and around the workspace; the whole matrix in ragged batches (int64 masks and packed
uint8 maps); a ragged batch against single calls, twice; the capacity, range and record statuses next to intact neighbours; the round
trip through hn_png_decode; hn_png_encode on the same inputs still png_enc_ref's streams.  Integer throughout: no tolerance."""
import io

import numpy as np
import pytest
import torch
from PIL import Image

from multitask_hydranet_amd import png, png_encode
from multitask_hydranet_amd._lib import lib
from tests import png_enc_dyn_ref as D
from tests import png_enc_ref as R

pytestmark = pytest.mark.gpu

SENT = 0xA5
GUARD = 4096                            # bytes before / behind every stream slot and the workspace
DEV = "cuda:0"
ENTRY = {"dynamic": ("hn_png_encode_dyn", "hn_png_enc_dyn_ws_bytes"), "fixed": ("hn_png_encode", "hn_png_enc_ws_bytes")}


def chunk():
    return int(lib().query("hn_png_enc_chunk_bytes"))


def encode_guarded(maps, out_sizes=None, caps=None, as_uint8=False, huffman="dynamic"):
    """one batch of class maps through the entry point into sentinel-filled buffers -> (streams, status words).  Every stream slot has a
    guard band on both sides, so has the workspace, and the result array is longer than the batch.  Asserts the guards, that a refused
    image's slot is untouched, and that nothing lands at or past a slot's capacity."""
    entry, ws_query = ENTRY[huffman]
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
    wsb = int(lib().query(ws_query, n, max_raw))
    assert wsb > 0
    ws = torch.full((GUARD + wsb + GUARD,), SENT, dtype=torch.uint8, device=DEV)
    result = torch.full((2 * (n + 4),), 77, dtype=torch.int64, device=DEV)
    desc_d = torch.from_numpy(desc.view(np.uint8).copy()).to(DEV)
    lib().call(entry, src.data_ptr(), int(src.numel()), 0 if as_uint8 else 1, desc_d.data_ptr(), n, max_h, max_raw,
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


def first_difference(a, b):
    k = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
    return k


def test_matrix_streams_equal_the_restatement():
    """every case of the matrix, int64 masks, in four ragged batches (case k goes to batch k mod 4)"""
    rows, _ = D.encoded_cases(chunk())
    wrong = []
    for b in range(4):
        sel = rows[b::4]
        streams, status = encode_guarded([r[1] for r in sel], [r[2] for r in sel])
        for r, s, st in zip(sel, streams, status):
            if st != r[4] or s != r[3]:
                wrong.append((r[0], st, len(s), len(r[3]), first_difference(s, r[3])))
    assert not wrong, "device streams differ (case, status, bytes, expected bytes, first differing byte): %s" % wrong[:16]


def test_packed_uint8_maps_give_the_same_streams():
    rows, _ = D.encoded_cases(chunk())
    sel = [r for r in rows if r[1].size < 20000]
    assert len(sel) > 30
    streams, status = encode_guarded([r[1] for r in sel], [r[2] for r in sel], as_uint8=True)
    assert status == [0] * len(sel)
    assert [r[0] for r, s in zip(sel, streams) if s != r[3]] == []


def test_fixed_entry_point_is_unchanged_on_the_new_cases():
    C = chunk()
    cases = D.dyn_cases(C)
    streams, status = encode_guarded([c[1] for c in cases], [c[2] for c in cases], huffman="fixed")
    assert status == [0] * len(cases)
    assert [c[0] for c, s in zip(cases, streams) if s != R.encode(c[1], c[2], C)[0]] == []


def test_ragged_batch_equals_single_calls_and_repeats():
    C = chunk()
    maps = [R.label_like(66, 1000, 33), R.noise_map(), R.signed_noise(2 * C - 1, 3)[None], R.rows_repeat(256, 4), np.array([[9]], np.int64),
            D.header_row(C)]
    sizes = [None, None, None, None, (3, 5), None]
    together, status = encode_guarded(maps, sizes)
    again, status2 = encode_guarded(maps, sizes)
    assert status == status2 == [0] * len(maps)
    assert together == again
    for i, m in enumerate(maps):
        alone, st = encode_guarded([m], [sizes[i]])
        assert st == [0] and alone[0] == together[i], i
        assert alone[0] == D.encode(m, sizes[i], C)[0], i


def test_capacity_one_word_below_the_stream_reports_full():
    C = chunk()
    maps = [R.label_like(40, 64, 7), R.label_like(66, 1000, 33), R.label_like(24, 40, 8)]
    want = [D.encode(m, None, C)[0] for m in maps]
    exact = (len(want[1]) + 3) // 4 * 4
    streams, status = encode_guarded(maps, caps=[None, exact, None])
    assert status == [0, 0, 0] and streams == want
    assert D.encode(maps[1], None, C, cap=exact - 4)[1] == D.ST_FULL
    streams, status = encode_guarded(maps, caps=[None, exact - 4, None])
    assert status == [0, png_encode.ST_FULL, 0]
    assert streams == [want[0], b"", want[2]]
    files = png_encode.encode_batch(maps, cap=[4096, exact - 4, 4096], device=DEV, huffman="dynamic")
    for f, m in zip(files, maps):
        with Image.open(io.BytesIO(f)) as im:
            assert im.mode == "L" and np.array_equal(np.asarray(im), m)
    assert png.idat_bytes(png.parse(files[0])) == want[0] and png.idat_bytes(png.parse(files[1])) == png_encode.host_stream(maps[1])


def test_range_and_record_statuses():
    C = chunk()
    good = R.label_like(24, 40, 8)
    bad = good.copy()
    bad[11, 17] = 256
    neg = good.copy()
    neg[0, 0] = -1
    want = D.encode(good, None, C)[0]
    streams, status = encode_guarded([good, bad, good, neg])
    assert status == [0, png_encode.ST_RANGE, 0, png_encode.ST_RANGE] and streams == [want, b"", want, b""]
    with pytest.raises(ValueError):
        png_encode.encode_batch([good, bad], device=DEV, huffman="dynamic")
    streams, status = encode_guarded([good, good, good], caps=[None, 1022, None])      # a capacity that is no multiple of 4
    assert status == [0, png_encode.ST_RECORD, 0] and streams == [want, b"", want]
    f = lib().raw("hn_png_encode_dyn")
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device=DEV)
    p = buf.data_ptr()
    assert f(p, 16, 1, p, 0, 1, 16, p, 1 << 16, p, 4096, p, None) == 1                   # N = 0
    assert f(p, 16, 1, p, 1, 1, 16, p, 16, p, 4096, p, None) == 1                        # a workspace that is too small
    assert f(p, 16, 1, p, 1, 1, 16, p, int(lib().query("hn_png_enc_ws_bytes", 1, 16)), p, 4096, p, None) == 1      # the fixed path's size
    assert f(p, 16, 2, p, 1, 1, 16, p, 1 << 16, p, 4096, p, None) == 1                   # no such source type
    assert f(p, 16, 1, p, 1, 1, 1 << 30, p, 1 << 16, p, 4096, p, None) == 1              # raw size out of range
    torch.cuda.synchronize()


def test_round_trip_through_the_device_decoder():
    """hn_png_decode reads what hn_png_encode_dyn writes: mixed fixed and dynamic blocks, the deepest codes, the 34-bit token"""
    C = chunk()
    rows = {r[0]: r for r in D.encoded_cases(C)[0][len(R.cases(C)):]}
    names = ["zero1x1", "chunks1", "chunks17", "chunks33", "header_runs", "cl_limit", "fibonacci", "label512up"]
    sel = [rows[k] for k in names]
    streams, status = encode_guarded([r[1] for r in sel], [r[2] for r in sel])
    assert status == [0] * len(sel)
    files = [png_encode.assemble(r[5].shape[1], r[5].shape[0], s) for r, s in zip(sel, streams)]
    back = png.imread_label_device(files, device=DEV)
    assert back["status"].cpu().tolist() == [0] * len(sel)
    flat = back["data"].cpu().numpy()
    for j, r in enumerate(sel):
        h, w = r[5].shape
        o = int(back["offsets"][j])
        assert tuple(back["shapes"][j]) == (h, w), r[0]
        assert np.array_equal(flat[o:o + h * w].reshape(h, w), r[5]), r[0]


def test_encode_batch_dynamic_files_and_bogus_code():
    C = chunk()
    mask = torch.from_numpy(np.stack([R.label_like(24, 40, s) for s in (1, 2, 3)])).to(DEV)
    grey = png_encode.encode_batch(mask, out_sizes=(45, 77), huffman="dynamic")
    pal = png_encode.encode_batch(mask, out_sizes=(45, 77), palette=R.PALETTE, huffman="dynamic")
    fixed = png_encode.encode_batch(mask, out_sizes=(45, 77))
    for k in range(3):
        stream, st, img, lines = D.encode(mask[k].cpu().numpy(), (45, 77), C)
        assert grey[k] == R.assemble(77, 45, stream) and pal[k] == R.assemble(77, 45, stream, R.PALETTE)
        assert fixed[k] == R.assemble(77, 45, R.encode(mask[k].cpu().numpy(), (45, 77), C)[0]) and len(grey[k]) <= len(fixed[k])
        for data, mode in ((grey[k], "L"), (pal[k], "P")):
            with Image.open(io.BytesIO(data)) as im:
                assert im.mode == mode and np.array_equal(np.asarray(im), img)
    for call in (png_encode.encode_batch, png_encode.encode_streams):
        with pytest.raises(ValueError):
            call(mask, huffman="bogus")
    with pytest.raises(ValueError):
        png_encode.imwrite("unused.png", mask[0], huffman="bogus")


def test_imwrite_dynamic(tmp_path):
    m = R.label_like(66, 1000, 33)
    png_encode.imwrite(str(tmp_path / "dyn.png"), m, device=DEV, huffman="dynamic")
    png_encode.imwrite(str(tmp_path / "fix.png"), m, device=DEV)
    with Image.open(str(tmp_path / "dyn.png")) as im:
        assert im.mode == "L" and np.array_equal(np.asarray(im), m)
    assert (tmp_path / "dyn.png").stat().st_size * 10 <= (tmp_path / "fix.png").stat().st_size * 6
