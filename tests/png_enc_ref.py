"""A numpy / Python restatement of the PNG label encode (hn_png_enc.hip through multitask_hydranet_amd/png_encode.py), stage by
stage, and the case matrix both test files walk.  Written from the formulation, not from the kernel: rows are filtered one at a time with
five small functions, the deflate parses every chunk with an explicit greedy loop, and the bits are packed with np.packbits.

  resize(m, (Ho, Wo))        cv2's INTER_NEAREST index rule in float64
  filter_rows(img)           H x (1 + W) filtered scanlines, the filter with the smallest sum of |int8| per row (ties: the lowest number)
  deflate(raw, S, C)         chunks of C raw bytes, each one fixed-Huffman block parsed greedily over the distances {1, S}
  zlib_stream(raw, S, C)     78 01 + the blocks + the big-endian Adler-32
  assemble(w, h, stream)     signature, IHDR, optional PLTE, one IDAT, IEND
  encode(m, out_hw, C, cap)  -> (stream, status, stats): what hn_png_encode leaves for one image
"""
import struct
import zlib

import numpy as np

ST_OK, ST_RANGE, ST_FULL = 0, 1, 2

LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEXT = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385,
         24577]
DEXT = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]


def resize(m, out_hw):
    hs, ws = m.shape
    ho, wo = out_hw
    out = np.empty((ho, wo), m.dtype)
    sx = [min(int(np.floor(np.float64(x) * (np.float64(1.0) / (np.float64(wo) / np.float64(ws))))), ws - 1) for x in range(wo)]
    for y in range(ho):
        sy = min(int(np.floor(np.float64(y) * (np.float64(1.0) / (np.float64(ho) / np.float64(hs))))), hs - 1)
        out[y] = m[sy, sx]
    return out


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def filter_rows(img):
    """-> (scanlines uint8 [H, 1 + W], the filter chosen for every row)"""
    h, w = img.shape
    out = np.zeros((h, 1 + w), np.uint8)
    zero = np.zeros(w, np.int64)
    for y in range(h):
        cur = img[y].astype(np.int64)
        up = img[y - 1].astype(np.int64) if y else zero
        left = np.concatenate([[0], cur[:-1]])
        upleft = np.concatenate([[0], up[:-1]])
        rows = [cur, cur - left, cur - up, cur - (left + up) // 2, cur - _paeth(left, up, upleft)]
        rows = [(r % 256).astype(np.uint8) for r in rows]
        costs = [int(np.abs(r.view(np.int8).astype(np.int64)).sum()) for r in rows]
        ft = costs.index(min(costs))
        out[y, 0] = ft
        out[y, 1:] = rows[ft]
    return out, [int(v) for v in out[:, 0]]


def _runs(eq):
    """eq[q] -> the count of consecutive true values starting at q"""
    n = len(eq)
    stop = np.where(eq, n, np.arange(n))
    return np.minimum.accumulate(stop[::-1])[::-1] - np.arange(n)


def _rev(code, n):
    return int(format(code, "0%db" % n)[::-1], 2)


def literal_bits(b):
    return (_rev(0x30 + b, 8), 8) if b < 144 else (_rev(0x190 + b - 144, 9), 9)


def length_symbol(length):
    idx = max(i for i in range(29) if LBASE[i] <= length)
    return idx, length - LBASE[idx]


def distance_symbol(dist):
    idx = max(i for i in range(30) if DBASE[i] <= dist)
    return idx, dist - DBASE[idx]


def match_bits(length, dist):
    idx, ext = length_symbol(length)
    sym = 257 + idx
    v, n = (_rev(sym - 256, 7), 7) if sym < 280 else (_rev(0xC0 + sym - 280, 8), 8)
    v |= ext << n
    n += LEXT[idx]
    di, dext = distance_symbol(dist)
    v |= _rev(di, 5) << n
    n += 5
    v |= dext << n
    n += DEXT[di]
    return v, n


def new_stats():
    return {"length_symbols": set(), "distance_codes": set(), "literal_low": 0, "literal_high": 0, "cross_chunk": 0, "filters": set(),
            "tokens": 0}


def deflate(raw, S, C, stats=None):
    """raw (uint8) -> the deflate bits as a list of (value, count) in stream order"""
    stats = stats if stats is not None else new_stats()
    raw = np.asarray(raw, np.uint8)
    n = len(raw)
    eq1 = np.zeros(n, bool)
    eq1[1:] = raw[1:] == raw[:-1]
    eqS = np.zeros(n, bool)
    if S <= 32768 and S < n:
        eqS[S:] = raw[S:] == raw[:-S]
    out = []
    for c0 in range(0, n, C):
        c1 = min(c0 + C, n)
        out.append(((1 if c1 == n else 0) | (1 << 1), 3))
        r1 = np.minimum(_runs(eq1[c0:c1]), 258)
        rS = np.minimum(_runs(eqS[c0:c1]), 258)
        p = 0
        while p < c1 - c0:
            l1, lS = int(r1[p]), int(rS[p])
            length, dist = (lS, S) if lS > l1 else (l1, 1)
            stats["tokens"] += 1
            if length >= 3:
                out.append(match_bits(length, dist))
                stats["length_symbols"].add(257 + length_symbol(length)[0])
                stats["distance_codes"].add(distance_symbol(dist)[0])
                if p - dist < 0:
                    stats["cross_chunk"] += 1
                p += length
            else:
                b = int(raw[c0 + p])
                out.append(literal_bits(b))
                stats["literal_low" if b < 144 else "literal_high"] += 1
                p += 1
        out.append((0, 7))
    return out


def pack_bits(tokens):
    vals = np.array([t[0] for t in tokens], np.uint64)
    cnts = np.array([t[1] for t in tokens], np.int64)
    start = np.concatenate([[0], np.cumsum(cnts)])
    bits = np.zeros((int(start[-1]) + 7) // 8 * 8, np.uint8)
    for j in range(int(cnts.max())):
        sel = cnts > j
        bits[start[:-1][sel] + j] = ((vals[sel] >> np.uint64(j)) & np.uint64(1)).astype(np.uint8)
    return np.packbits(bits, bitorder="little").tobytes()


def zlib_stream(raw, S, C, stats=None):
    raw = np.asarray(raw, np.uint8).reshape(-1)
    return b"\x78\x01" + pack_bits(deflate(raw, S, C, stats)) + struct.pack(">I", zlib.adler32(raw.tobytes()) & 0xFFFFFFFF)


def capacity(raw_bytes, C):
    blocks = (raw_bytes + C - 1) // C
    return (2 + (9 * raw_bytes + 10 * blocks + 7) // 8 + 4 + 15) // 16 * 16


def encode(m, out_hw, C, cap=None, stats=None):
    """one class map (any integer dtype) -> (stream, status, the resized uint8 map, the scanlines)"""
    m = np.asarray(m)
    out_hw = tuple(out_hw) if out_hw is not None else m.shape
    big = resize(m.astype(np.int64), out_hw)
    if big.min() < 0 or big.max() > 255:
        return b"", ST_RANGE, None, None
    img = big.astype(np.uint8)
    lines, filters = filter_rows(img)
    if stats is not None:
        stats["filters"].update(filters)
    stream = zlib_stream(lines, img.shape[1] + 1, C, stats)
    if cap is not None and len(stream) > cap:
        return b"", ST_FULL, img, lines
    return stream, ST_OK, img, lines


def _chunk(kind, payload):
    return struct.pack(">I", len(payload)) + kind + payload + struct.pack(">I", zlib.crc32(kind + payload) & 0xFFFFFFFF)


def assemble(width, height, stream, palette=None):
    out = b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", width, height, 8, 0 if palette is None else 3, 0, 0, 0))
    if palette is not None:
        table = bytearray(3 * (max(palette) + 1))
        for k, (r, g, b) in palette.items():
            table[3 * k:3 * k + 3] = bytes([r, g, b])
        out += _chunk(b"PLTE", bytes(table))
    return out + _chunk(b"IDAT", stream) + _chunk(b"IEND", b"")


# ------------------------------------------------------------------------------------------------ the case matrix

S_EDGES = (4, 5, 8, 9, 16, 17, 32, 33, 256, 257, 1024, 1025, 4096, 4097, 24576, 24577, 32768, 32769)
ZERO_RUNS = (2, 3, 4, 10, 11, 257, 258, 259, 260, 261, 516)
PALETTE = {0: (0, 0, 0), 1: (128, 0, 128), 2: (255, 255, 255), 3: (0, 255, 255), 4: (0, 255, 0)}


def _rng(seed):
    return np.random.Generator(np.random.Philox(seed))


def rows_repeat(width, seed, height=3):
    """rows whose Up-filtered form repeats from row 1 on (the same small steps every row) without being constant: the row distance wins"""
    g = _rng(seed)
    step = g.integers(0, 2, size=width)
    step[::3] = 2 - step[::3]
    rows = [g.integers(0, 5, size=width)]
    for _ in range(height - 1):
        rows.append((rows[-1] + step) % 256)
    return np.stack(rows).astype(np.int64)


def signed_noise(width, seed):
    """one row that the None filter wins: +1 / +2 on even columns, -1 / -2 on odd ones"""
    g = _rng(seed)
    v = g.integers(1, 3, size=width)
    v[1::2] = 256 - v[1::2]
    return v.astype(np.int64)


def zero_run_row(C, start, length, seed):
    """one row of 2 C + 10 pixels whose scanline has `length` zero bytes from raw position `start`"""
    row = signed_noise(2 * C + 10, seed)
    row[start - 1:start - 1 + length] = 0
    return row[None]


def all_lengths_row(seed):
    """zero runs that give a match of every base length 3 .. 258, apart"""
    parts = []
    for k, base in enumerate(LBASE):
        parts += [signed_noise(6, seed + k), np.zeros(base + 1, np.int64)]
    parts.append(signed_noise(6, seed + 99))
    return np.concatenate(parts)[None]


def stripes(h, w, seed):
    """vertical stripes in the left half, horizontal ones in the right: Paeth predicts both"""
    g = _rng(seed)
    a, b = g.integers(0, 256, size=w), g.integers(0, 256, size=h)
    m = np.empty((h, w), np.int64)
    m[:, :w // 2] = a[None, :w // 2]
    m[:, w // 2:] = b[:, None]
    return m


def label_like(h, w, seed, classes=5):
    """large constant regions with ragged boundaries"""
    g = _rng(seed)
    m = np.zeros((h, w), np.int64)
    for k in range(1, classes):
        edge = np.cumsum(g.integers(-2, 3, size=h)) + g.integers(w // 8, w - w // 8)
        m[np.arange(w)[None, :] > edge[:, None]] = k
    return m


def noise_map(h=37, w=53, seed=11):
    return _rng(seed).integers(0, 256, size=(h, w)).astype(np.int64)


def cases(C):
    """-> list of (name, int64 map, out_hw or None)"""
    out = [("1x1", np.array([[7]], np.int64), None), ("1x7", signed_noise(7, 1)[None], None), ("7x1", signed_noise(7, 2)[:, None], None)]
    widths = sorted(set([s - 1 for s in S_EDGES] + [d - 1 for d in DBASE[2:]]))
    for k, w in enumerate(widths):
        out.append(("S%d" % (w + 1), rows_repeat(w, 100 + k), None))
    yy, xx = np.mgrid[0:12, 0:2]
    out.append(("S2", (3 * yy[:, :1]) % 256, None))                     # scanlines 2, 3, 2, 3, ...: distance 2
    out.append(("S3", (3 * yy + 7 * xx) % 256, None))
    for w in (C - 2, C - 1, C, 2 * C - 1):
        out.append(("raw%d" % (w + 1), signed_noise(w, 200 + w % 7)[None], None))
    for k, n in enumerate(ZERO_RUNS):
        out.append(("zeros%d@start" % n, zero_run_row(C, C, n, 300 + k), None))
        out.append(("zeros%d@straddle" % n, zero_run_row(C, 2 * C - n // 2, n, 330 + k), None))
    out.append(("lengths", all_lengths_row(400), None))
    edge = np.tile(np.array([143, 144, 255, 144, 143, 255, 255, 143], np.int64), (4, 9))
    edge[1::2] = np.roll(edge[1::2], 3, axis=1)
    out.append(("values", edge, None))
    out.append(("periodS", np.tile(_rng(5).integers(0, 256, size=(1, 61)), (5, 1)).astype(np.int64), None))
    yy, xx = np.mgrid[0:9, 0:70]
    out.append(("ramp_sub", (3 * xx) % 256, None))
    out.append(("ramp_avg", (3 * xx - 3 * yy) % 256, None))
    out.append(("stripes_paeth", stripes(12, 80, 6), None))
    out.append(("noise", noise_map(), None))
    out.append(("label", label_like(40, 64, 7), None))
    out.append(("up45x77", label_like(24, 40, 8), (45, 77)))
    out.append(("same24x40", label_like(24, 40, 9), (24, 40)))
    out.append(("down", label_like(40, 64, 10), (13, 21)))
    return out


_ENCODED = {}


def encoded_cases(C):
    """the matrix through encode(), computed once per chunk size: (list of (name, map, out_hw, stream, status, resized map, scanlines), stats)"""
    if C not in _ENCODED:
        stats = new_stats()
        rows = []
        for name, m, out_hw in cases(C):
            stream, status, img, lines = encode(m, out_hw, C, stats=stats)
            rows.append((name, m, out_hw, stream, status, img, lines))
        _ENCODED[C] = (rows, stats)
    return _ENCODED[C]
