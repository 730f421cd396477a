"""The PNG label encode without a GPU: the numpy restatement (tests/png_enc_ref.py) is held to independent decoders over the whole case
matrix -- zlib inflates every stream to the restatement's own scanlines, PIL opens every assembled file and returns the resized map,
png.parse accepts it with every CRC good -- and the matrix is shown to reach every branch the formulation names.  png_encode's host parts
(assemble, the per-image fallback) are tested directly.  Exact throughout."""
import io
import zlib

import numpy as np
from PIL import Image

from multitask_hydranet_amd import png, png_encode
from multitask_hydranet_amd._lib import lib
from tests import png_enc_ref as R


def chunk():
    return int(lib().query("hn_png_enc_chunk_bytes"))


def pil_array(data):
    with Image.open(io.BytesIO(data)) as im:
        im.load()
        return im.mode, np.asarray(im).copy(), im.getpalette()


def test_chunk_size_and_capacity_formula():
    C = chunk()
    assert 512 <= C <= 32768
    for raw in (1, 2, C - 1, C, C + 1, 2 * C, 1080 * 1921):
        want = 2 + -(-(9 * raw + 10 * -(-raw // C)) // 8) + 4
        got = int(lib().query("hn_png_enc_cap_bytes", raw))
        assert want <= got < want + 16 and got % 16 == 0, (raw, want, got)
        assert got == R.capacity(raw, C)
    assert int(lib().query("hn_png_enc_cap_bytes", 0)) == -1 and int(lib().query("hn_png_enc_ws_bytes", 0, 100)) == -1
    assert int(lib().query("hn_png_enc_ws_bytes", 3, 1 << 30)) == -1 and int(lib().query("hn_png_enc_ws_bytes", 3, 5000)) > 3 * 5008


def test_restatement_streams_inflate_to_their_scanlines():
    rows, _ = R.encoded_cases(chunk())
    assert len(rows) >= 70
    for name, m, out_hw, stream, status, img, lines in rows:
        assert status == R.ST_OK, name
        assert stream[:2] == b"\x78\x01", name
        assert zlib.decompress(stream) == lines.tobytes(), name
        assert len(stream) <= R.capacity(lines.size, chunk()), name


def test_restatement_files_open_in_pil_and_parse():
    rows, _ = R.encoded_cases(chunk())
    for name, m, out_hw, stream, status, img, lines in rows:
        h, w = img.shape
        want = R.resize(m, out_hw or m.shape).astype(np.uint8)
        assert np.array_equal(img, want), name
        data = R.assemble(w, h, stream)
        mode, arr, _ = pil_array(data)
        assert mode == "L" and np.array_equal(arr, want), name
        head = png.parse(data)                                            # verifies every chunk's CRC
        assert head is not None and (head["width"], head["height"], head["color_type"], head["bpp"]) == (w, h, 0, 1), name
        assert png.idat_bytes(head) == stream and head["raw_bytes"] == lines.size, name
        assert data == png_encode.assemble(w, h, stream), name


def test_palette_variant_same_indices():
    rows, _ = R.encoded_cases(chunk())
    pick = [r for r in rows if r[0] in ("label", "up45x77", "1x1")]
    assert len(pick) == 3
    for name, m, out_hw, stream, status, img, lines in pick:
        h, w = img.shape
        data = R.assemble(w, h, stream, R.PALETTE)
        assert data == png_encode.assemble(w, h, stream, R.PALETTE), name
        mode, arr, pal = pil_array(data)
        assert mode == "P" and np.array_equal(arr, img), name
        assert pal[:15] == [v for k in range(5) for v in R.PALETTE[k]], name
        head = png.parse(data)
        assert head is not None and head["color_type"] == 3 and png.idat_bytes(head) == stream, name
        assert np.array_equal(png.pil_label(data), img), name


def test_matrix_reaches_every_branch():
    C = chunk()
    _, st = R.encoded_cases(C)
    assert st["length_symbols"] == set(range(257, 286)), sorted(set(range(257, 286)) - st["length_symbols"])
    assert st["distance_codes"] == set(range(30)), sorted(set(range(30)) - st["distance_codes"])
    assert st["literal_low"] > 0 and st["literal_high"] > 0
    assert st["filters"] == {0, 1, 2, 3, 4}, st["filters"]
    assert st["cross_chunk"] > 0
    # S = 32769 switches the row candidate off: only distance 1 there
    own = R.new_stats()
    R.encode(R.rows_repeat(32768, 1), None, C, stats=own)
    assert own["distance_codes"] <= {0}, own["distance_codes"]


def test_constant_map_is_coded_with_matches():
    """64 x 1000 constant non-zero map: at most raw / 32 (a zero chunk costs one literal and 258-byte matches of 13 bits, about raw / 70;
    the rest is room for the first row and the chunk tails): a literal-only coder cannot meet it"""
    C = chunk()
    m = np.full((64, 1000), 3, np.int64)
    stream, status, img, lines = R.encode(m, None, C)
    assert status == 0 and zlib.decompress(stream) == lines.tobytes()
    assert len(stream) * 32 <= lines.size, (len(stream), lines.size)


def test_restatement_resize_rule():
    m = np.arange(6 * 5, dtype=np.int64).reshape(6, 5)
    assert np.array_equal(R.resize(m, (6, 5)), m)
    for hw in ((45, 77), (13, 3), (1, 1), (7, 11)):
        got = R.resize(m, hw)
        sx = [min(int(np.floor(x * (1.0 / (hw[1] / 5)))), 4) for x in range(hw[1])]
        sy = [min(int(np.floor(y * (1.0 / (hw[0] / 6)))), 5) for y in range(hw[0])]
        assert np.array_equal(got, m[np.ix_(sy, sx)]), hw
        assert np.array_equal(png_encode.resize_nearest(m, hw), got), hw


def test_assemble_layout():
    stream = zlib.compress(bytes([0, 5, 0, 6]))
    data = png_encode.assemble(1, 2, stream)
    assert data[:8] == png.SIGNATURE and data[12:16] == b"IHDR" and data[-12:-8] == b"\x00\x00\x00\x00" and data[-8:-4] == b"IEND"
    head = png.parse(data)
    assert head["idat"] == [(8 + 25 + 8, len(stream))] and len(head["idat"]) == 1
    mode, arr, _ = pil_array(data)
    assert mode == "L" and arr.tolist() == [[5], [6]]
    assert png_encode.palette_bytes({0: (1, 2, 3), 2: (7, 8, 9)}) == bytes([1, 2, 3, 0, 0, 0, 7, 8, 9])


def test_host_fallback_matches_the_restatement_filters():
    rows, _ = R.encoded_cases(chunk())
    for name, m, out_hw, stream, status, img, lines in rows:
        if m.size > 20000:
            continue
        assert np.array_equal(png_encode.filter_rows(img), lines), name
        s = png_encode.host_stream(m, out_hw)
        assert zlib.decompress(s) == lines.tobytes(), name
        mode, arr, _ = pil_array(png_encode.encode_host(m, out_hw))
        assert mode == "L" and np.array_equal(arr, img), name
    mode, arr, pal = pil_array(png_encode.encode_host(R.label_like(9, 14, 3), (20, 31), R.PALETTE))
    assert mode == "P" and np.array_equal(arr, R.resize(R.label_like(9, 14, 3), (20, 31)))


def test_host_fallback_refuses_out_of_range_ids():
    import pytest
    bad = np.zeros((4, 4), np.int64)
    bad[2, 1] = 256
    with pytest.raises(ValueError):
        png_encode.host_stream(bad)
    bad[2, 1] = -1
    with pytest.raises(ValueError):
        png_encode.host_stream(bad)
    assert R.encode(np.full((2, 2), 256, np.int64), None, chunk())[1] == R.ST_RANGE
