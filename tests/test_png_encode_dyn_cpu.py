"""The dynamic-Huffman PNG label encode without a GPU: the restatement (tests/png_enc_dyn_ref.py) is held to independent decoders over
png_enc_ref's whole case matrix and the cases the block layer adds -- zlib inflates every stream to the scanlines, PIL opens every
assembled file and returns the resized map, no stream is longer than the fixed-code one -- and the matrix's statistics are shown to reach
every branch of the block layer, so that a case that misses its target fails here and not on the GPU.  Exact throughout.

Two items of the coverage list cannot occur under the header rules as they are fixed, and are replaced by the nearest that can:
  HCLEN 4: the two distance lengths are always 1, so code-length symbol 1 -- entry 18 of the RFC's order -- is always used: HCLEN is 18 or
    19, and both are required here.
  a run-length symbol that covers literal/length AND distance lengths: the last literal/length entry is a used symbol (non-zero), the
    first distance length is 1, and a repeat symbol needs four equal lengths, which only the pair {255, end of block} could give; every
    block holds a filter byte (0..4), so that block does not exist.  Required instead: a run measured from a literal/length position
    that extends into the distance lengths (the sequence is walked as one)."""
import io
import zlib

import numpy as np
from PIL import Image

from multitask_hydranet_amd._lib import lib
from tests import png_enc_dyn_ref as D
from tests import png_enc_ref as R


def chunk():
    return int(lib().query("hn_png_enc_chunk_bytes"))


def test_block_size_and_workspace_queries():
    assert int(lib().query("hn_png_enc_block_chunks")) == D.BLOCK_CHUNKS == 16
    C = chunk()
    for n, raw in ((1, 1), (3, 5000), (16, 1080 * 1921)):
        assert int(lib().query("hn_png_enc_dyn_ws_bytes", n, raw)) > int(lib().query("hn_png_enc_ws_bytes", n, raw)) + n * -(-raw // C) * 286 * 4
    assert int(lib().query("hn_png_enc_dyn_ws_bytes", 0, 100)) == -1 and int(lib().query("hn_png_enc_dyn_ws_bytes", 3, 1 << 30)) == -1


def test_streams_inflate_open_in_pil_and_are_no_longer_than_fixed():
    C = chunk()
    rows, _ = D.encoded_cases(C)
    fixed = [r[3] for r in R.encoded_cases(C)[0]]                           # png_enc_ref's cases come first, in its order
    assert len(rows) >= 80
    for k, (name, m, out_hw, stream, status, img, lines) in enumerate(rows):
        assert status == D.ST_OK and stream[:2] == b"\x78\x01", name
        assert zlib.decompress(stream) == lines.tobytes(), name
        want = R.resize(m, out_hw or m.shape).astype(np.uint8)
        with Image.open(io.BytesIO(R.assemble(img.shape[1], img.shape[0], stream))) as im:
            assert im.mode == "L" and np.array_equal(np.asarray(im), want), name
        ref = fixed[k] if k < len(fixed) else R.encode(m, out_hw, C)[0]
        assert len(stream) <= len(ref) <= R.capacity(lines.size, C), (name, len(stream), len(ref))


def test_matrix_reaches_every_branch_of_the_block_layer():
    C = chunk()
    _, st = D.encoded_cases(C)
    print({k: (sorted(v) if isinstance(v, set) else v) for k, v in st.items()})
    assert st["fixed_blocks"] > 0 and st["dynamic_blocks"] > 0 and st["mixed_images"] > 0
    assert {1, 16, 17, 33} <= st["image_chunks"], sorted(st["image_chunks"])
    assert {1, 16} <= st["last_block_chunks"] and st["mid_row_block_edge"] > 0
    assert {(16, 3), (16, 6), (17, 3), (17, 10), (18, 11), (18, 138)} <= st["rle"], sorted(st["rle"])
    assert 139 in st["zero_runs"] and {1, 2} <= st["zero_runs"], sorted(st["zero_runs"])
    assert st["run_into_dist"] > 0
    assert {257, 286} <= st["hlit"], sorted(st["hlit"])
    assert st["hclen"] == {18, 19}, sorted(st["hclen"])
    assert st["ll_depth"] >= 16 and st["cl_depth"] >= 8, (st["ll_depth"], st["cl_depth"])
    assert st["big_S"] > 0
    assert st["token_bits"] >= 33, st["token_bits"]


def one(name):
    C = chunk()
    case = [c for c in D.dyn_cases(C) if c[0] == name]
    assert len(case) == 1
    st = D.new_stats()
    stream, status, img, lines = D.encode(case[0][1], case[0][2], C, stats=st)
    return case[0][1], stream, lines, st


def test_the_cases_do_what_they_claim():
    C = chunk()
    m, stream, lines, st = one("fibonacci")
    assert set(lines[:, 0].tolist()) == {0}                                 # the None filter on every row
    assert m.shape[1] >= 16384 and len(np.unique(lines[:, 1:])) >= 17
    assert st["ll_depth"] >= 16 and 19 in st["hclen"] and st["token_bits"] >= 33 and st["dynamic_blocks"] == 2
    toks = [t for ch in D.parse(lines.reshape(-1), m.shape[1] + 1, C) for t in ch if t[0] == "match"]
    long = [t for t in toks if t[1] >= 131]                                  # the planted row match, once: its length symbol is the rarest
    assert len(long) == 1 and long[0][1] <= 257 and long[0][2] == m.shape[1] + 1, toks
    m, stream, lines, st = one("cl_limit")
    assert set(lines[:, 0].tolist()) == {0} and st["cl_depth"] >= 8 and st["dynamic_blocks"] == 1
    m, stream, lines, st = one("header_runs")
    assert set(lines[:, 0].tolist()) == {0} and 139 in st["zero_runs"]
    assert {(16, 3), (16, 6), (17, 3), (17, 10), (18, 11), (18, 138)} <= st["rle"], sorted(st["rle"])
    m, stream, lines, st = one("chunks17")
    assert st["image_chunks"] == {17} and st["mixed_images"] == 1 and st["last_block_chunks"] == {1} and st["mid_row_block_edge"] == 1
    m, stream, lines, st = one("noise17")
    assert st["image_chunks"] == {17} and st["mixed_images"] == 1 and st["hlit"] == {257} and st["big_S"] == 1
    for name, n in (("chunks1", 1), ("chunks16", 16), ("chunks33", 33)):
        m, stream, lines, st = one(name)
        assert st["image_chunks"] == {n} and lines.size <= n * C, name
    assert one("chunks1")[2].size == C
    m, stream, lines, st = one("zero1x1")
    assert st["run_into_dist"] == 1 and st["fixed_blocks"] == 1 and stream == R.encode(m, None, C)[0]
    m, stream, lines, st = one("bigS")
    assert st["big_S"] == 1 and st["dynamic_blocks"] == 2


def test_huffman_routine_properties():
    """complete codes within the limit, deterministic ties, the single-symbol rule; Fibonacci counts reach depth n - 1"""
    for n in (17, 20, 22):
        lens, depth = D.huffman_lengths(D.FIB[:n], 15)                      # 1, 1, 2, 3, 5, ...: one chain
        assert depth == n - 1 and max(lens) == min(15, n - 1)
        assert sum(1 << (15 - l) for l in lens if l) == 1 << 15
    assert D.huffman_lengths([0, 5, 0], 7) == ([0, 1, 0], 1)
    assert D.huffman_lengths([3, 3, 3, 3], 7)[0] == [2, 2, 2, 2]
    lens, depth = D.huffman_lengths([1, 1, 2, 3, 5, 8, 13, 21, 34], 7)
    assert depth == 8 and max(lens) == 7 and sum(1 << (7 - l) for l in lens) == 1 << 7
    assert lens == sorted(lens, reverse=True)                               # the larger count never has the longer code
    g = R._rng(3)
    for _ in range(50):
        counts = (g.integers(0, 4, size=286) * g.integers(0, 3000, size=286)).tolist()
        counts[256] = 1
        lens, _ = D.huffman_lengths(counts, 15)
        assert sum(1 << (15 - l) for l in lens if l) == 1 << 15 and all((l > 0) == (c > 0) for l, c in zip(lens, counts))
        codes = D.canonical(lens)
        words = sorted(format(c, "0%db" % l) for c, l in zip(codes, lens) if l)
        assert all(not b.startswith(a) for a, b in zip(words, words[1:]))   # prefix-free


def test_label_map_at_1080p_is_at_most_six_tenths_of_the_fixed_stream():
    C = chunk()
    m = R.label_like(1080, 1920, 7)
    dyn, st, img, lines = D.encode(m, None, C)
    fixed = R.encode(m, None, C)[0]
    print("label_like(1080, 1920, 7): dynamic %d B, fixed %d B, zlib level 6 %d B" % (len(dyn), len(fixed), len(zlib.compress(lines.tobytes(), 6))))
    assert st == 0 and zlib.decompress(dyn) == lines.tobytes()
    assert len(dyn) <= 0.6 * len(fixed), (len(dyn), len(fixed))
