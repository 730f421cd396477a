"""A numpy / Python restatement of the PNG label encode with dynamic-Huffman blocks (hn_png_encode_dyn in hn_png_enc.hip):
the definition the kernels are held to, bit for bit.  Resize, row filters, the per-chunk greedy parse and the case matrix are
tests/png_enc_ref.py's; what is new is the block layer, written from RFC 1951 3.2.7 with plain lists and sorted().

  parse(raw, S, C)                 per chunk of C raw bytes the tokens ("lit", byte) / ("match", length, distance), the fixed path's parse
  huffman_lengths(counts, limit)   two-queue Huffman over the used symbols (leaves by (count, symbol); a leaf before an internal node of
                                   equal weight), depths clamped to `limit`, the Kraft sum repaired one unit a step (take one code from
                                   `limit`, split one code of the longest shorter length in two), lengths handed back by (count descending,
                                   symbol ascending), shortest first.  One used symbol: length 1.
  canonical(lengths)               RFC 1951 3.2.2 codes
  rle(seq)                         the code-length symbols of literal/length + distance lengths as ONE sequence, greedy from the left
  block_plan(tokens, S, final)     header bits, the two bit totals and the choice (dynamic only when strictly smaller) for one block of
                                   BLOCK_CHUNKS chunks
  zlib_stream / encode             78 01 + one block per 16 chunks + the big-endian Adler-32

The distance code is always two codes of length 1: code 0 (distance 1) and the code of the row distance S = Wo + 1 (code 1 when
S > 32768, where the parse takes no row matches)."""
import struct
import zlib

import numpy as np

from tests import png_enc_ref as R

ST_OK, ST_RANGE, ST_FULL = R.ST_OK, R.ST_RANGE, R.ST_FULL
BLOCK_CHUNKS = 16
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


def new_stats():
    return {"fixed_blocks": 0, "dynamic_blocks": 0, "mixed_images": 0, "image_chunks": set(), "rle": set(), "run_into_dist": 0,
            "hlit": set(), "hclen": set(), "ll_depth": 0, "cl_depth": 0, "big_S": 0, "token_bits": 0, "mid_row_block_edge": 0,
            "last_block_chunks": set(), "zero_runs": set()}


def parse(raw, S, C):
    """-> per chunk a list of tokens: ("lit", byte) or ("match", length, distance).  png_enc_ref.deflate's loop without the bits."""
    raw = np.asarray(raw, np.uint8)
    n = len(raw)
    eq1 = np.zeros(n, bool)
    eq1[1:] = raw[1:] == raw[:-1]
    eqS = np.zeros(n, bool)
    if S <= 32768 and S < n:
        eqS[S:] = raw[S:] == raw[:-S]
    chunks = []
    for c0 in range(0, n, C):
        c1 = min(c0 + C, n)
        r1 = np.minimum(R._runs(eq1[c0:c1]), 258).tolist()
        rS = np.minimum(R._runs(eqS[c0:c1]), 258).tolist()
        part = raw[c0:c1].tolist()
        toks, p = [], 0
        while p < c1 - c0:
            l1, lS = r1[p], rS[p]
            length, dist = (lS, S) if lS > l1 else (l1, 1)
            if length >= 3:
                toks.append(("match", length, dist))
                p += length
            else:
                toks.append(("lit", part[p]))
                p += 1
        chunks.append(toks)
    return chunks


def huffman_lengths(counts, limit):
    """-> (code lengths, the depth of the unrestricted tree)"""
    used = [s for s, c in enumerate(counts) if c > 0]
    lens = [0] * len(counts)
    if len(used) == 1:
        lens[used[0]] = 1
        return lens, 1
    leaves = sorted(used, key=lambda s: (counts[s], s))
    m = len(leaves)
    weight = [counts[s] for s in leaves] + [0] * (m - 1)
    parent = [0] * (2 * m - 1)
    i, j = 0, m
    for k in range(m, 2 * m - 1):
        pair = []
        for _ in range(2):
            if i < m and (j >= k or weight[i] <= weight[j]):
                pair.append(i)
                i += 1
            else:
                pair.append(j)
                j += 1
        weight[k] = weight[pair[0]] + weight[pair[1]]
        parent[pair[0]] = parent[pair[1]] = k
    depth = [0] * (2 * m - 1)
    for node in range(2 * m - 3, -1, -1):
        depth[node] = depth[parent[node]] + 1
    deepest = max(depth[:m])
    bl = [0] * (limit + 1)
    for d in depth[:m]:
        bl[min(d, limit)] += 1
    kraft = sum(bl[l] << (limit - l) for l in range(1, limit + 1))
    while kraft > (1 << limit):
        bl[limit] -= 1
        b = limit - 1
        while bl[b] == 0:
            b -= 1
        bl[b] -= 1
        bl[b + 1] += 2
        kraft -= 1
    assert kraft == (1 << limit) and min(bl) >= 0
    length = 1
    for s in sorted(used, key=lambda s: (-counts[s], s)):
        while bl[length] == 0:
            length += 1
        lens[s] = length
        bl[length] -= 1
    return lens, deepest


def canonical(lens):
    """-> codes (MSB-first values, RFC 1951 3.2.2)"""
    top = max(lens)
    count = [0] * (top + 2)
    for l in lens:
        if l:
            count[l] += 1
    nxt, code = [0] * (top + 2), 0
    for l in range(1, top + 1):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    out = [0] * len(lens)
    for s, l in enumerate(lens):
        if l:
            out[s] = nxt[l]
            nxt[l] += 1
    return out


def rle(seq, hlit=None, stats=None):
    """-> list of (code-length symbol, extra value, extra bits)"""
    out, i, n = [], 0, len(seq)
    while i < n:
        v, run = seq[i], 1
        while i + run < n and seq[i + run] == v:
            run += 1
        if stats is not None and hlit is not None and i < hlit < i + run:
            stats["run_into_dist"] += 1
        if v == 0:
            if stats is not None:
                stats["zero_runs"].add(run)
            if run >= 11:
                k = min(run, 138)
                out.append((18, k - 11, 7))
                i += k
            elif run >= 3:
                out.append((17, run - 3, 3))
                i += run
            else:
                out.append((0, 0, 0))
                i += 1
        else:
            out.append((v, 0, 0))
            i += 1
            r = run - 1
            while r >= 3:
                k = min(r, 6)
                out.append((16, k - 3, 2))
                i += k
                r -= k
    return out


def distance_code(S):
    """the second distance code (the first is code 0, distance 1)"""
    return R.distance_symbol(S)[0] if S <= 32768 else 1


def block_plan(chunks, S, final, stats=None):
    """chunks: the token lists of one block -> dict with the choice and everything the writer needs"""
    hist = [0] * 286
    fixed_bits = extra = matches = 0
    for toks in chunks:
        for t in toks:
            if t[0] == "lit":
                hist[t[1]] += 1
                fixed_bits += R.literal_bits(t[1])[1]
            else:
                idx = R.length_symbol(t[1])[0]
                hist[257 + idx] += 1
                matches += 1
                extra += R.LEXT[idx] + (R.DEXT[R.distance_symbol(t[2])[0]] if t[2] != 1 else 0)
                fixed_bits += R.match_bits(t[1], t[2])[1]
    hist[256] = 1
    ll, ll_depth = huffman_lengths(hist, 15)
    dsym = distance_code(S)
    dl = [0] * (dsym + 1)
    dl[0] = dl[dsym] = 1
    hlit = max(s for s in range(286) if ll[s]) + 1
    assert hlit >= 257
    syms = rle(ll[:hlit] + dl, hlit, stats)
    clhist = [0] * 19
    for s, _, _ in syms:
        clhist[s] += 1
    cl, cl_depth = huffman_lengths(clhist, 7)
    hclen = max(4, max(k for k in range(19) if cl[CL_ORDER[k]]) + 1)
    clcode = canonical(cl)
    head = [(hlit - 257, 5), (dsym, 5), (hclen - 4, 4)] + [(cl[CL_ORDER[k]], 3) for k in range(hclen)]
    for s, ev, eb in syms:
        head.append((R._rev(clcode[s], cl[s]) | (ev << cl[s]), cl[s] + eb))
    head_bits = sum(nb for _, nb in head)
    dyn_tokens = sum(hist[s] * ll[s] for s in range(286)) - ll[256] + extra + matches
    dyn_bits = 3 + head_bits + dyn_tokens + ll[256]
    fix_bits = 3 + fixed_bits + 7
    dynamic = dyn_bits < fix_bits
    if stats is not None:
        stats["dynamic_blocks" if dynamic else "fixed_blocks"] += 1
        stats["hlit"].add(hlit)
        stats["hclen"].add(hclen)
        stats["ll_depth"] = max(stats["ll_depth"], ll_depth)
        stats["cl_depth"] = max(stats["cl_depth"], cl_depth)
        stats["rle"].update((s, ev + {16: 3, 17: 3, 18: 11}[s]) for s, ev, _ in syms if s >= 16)
    return {"dynamic": dynamic, "final": final, "ll": ll, "llcode": canonical(ll), "dsym": dsym, "head": head, "bits": min(dyn_bits, fix_bits)}


def block_bits(chunks, plan, S, stats=None):
    """-> the block's (value, count) list in stream order"""
    out = [((1 if plan["final"] else 0) | ((2 if plan["dynamic"] else 1) << 1), 3)]
    if not plan["dynamic"]:
        for toks in chunks:
            out += [R.literal_bits(t[1]) if t[0] == "lit" else R.match_bits(t[1], t[2]) for t in toks]
        out.append((0, 7))
        return out
    ll, code = plan["ll"], plan["llcode"]
    out += plan["head"]
    for toks in chunks:
        for t in toks:
            if t[0] == "lit":
                out.append((R._rev(code[t[1]], ll[t[1]]), ll[t[1]]))
                continue
            idx, ext = R.length_symbol(t[1])
            s = 257 + idx
            v, n = R._rev(code[s], ll[s]) | (ext << ll[s]), ll[s] + R.LEXT[idx]
            if t[2] == 1:
                d, dn = 0, 1
            else:
                di, dext = R.distance_symbol(t[2])
                d, dn = 1 | (dext << 1), 1 + R.DEXT[di]
            out.append((v | (d << n), n + dn))
            if stats is not None:
                stats["token_bits"] = max(stats["token_bits"], n + dn)
    out.append((R._rev(code[256], ll[256]), ll[256]))
    return out


def deflate(raw, S, C, stats=None):
    chunks = parse(raw, S, C)
    out, kinds = [], set()
    for b0 in range(0, len(chunks), BLOCK_CHUNKS):
        blk = chunks[b0:b0 + BLOCK_CHUNKS]
        plan = block_plan(blk, S, b0 + BLOCK_CHUNKS >= len(chunks), stats)
        bits = block_bits(blk, plan, S, stats)
        assert sum(nb for _, nb in bits) == plan["bits"]
        out += bits
        kinds.add(plan["dynamic"])
    if stats is not None:
        stats["image_chunks"].add(len(chunks))
        stats["last_block_chunks"].add((len(chunks) - 1) % BLOCK_CHUNKS + 1)
        stats["mixed_images"] += len(kinds) == 2
        stats["big_S"] += S > 32768
        stats["mid_row_block_edge"] += len(chunks) > BLOCK_CHUNKS and (BLOCK_CHUNKS * C) % S != 0
    return out


def zlib_stream(raw, S, C, stats=None):
    raw = np.asarray(raw, np.uint8).reshape(-1)
    return b"\x78\x01" + R.pack_bits(deflate(raw, S, C, stats)) + struct.pack(">I", zlib.adler32(raw.tobytes()) & 0xFFFFFFFF)


def encode(m, out_hw, C, cap=None, stats=None):
    """one class map (any integer dtype) -> (stream, status, the resized uint8 map, the scanlines): what hn_png_encode_dyn leaves"""
    m = np.asarray(m)
    out_hw = tuple(out_hw) if out_hw is not None else m.shape
    big = R.resize(m.astype(np.int64), out_hw)
    if big.min() < 0 or big.max() > 255:
        return b"", ST_RANGE, None, None
    img = big.astype(np.uint8)
    lines, _ = R.filter_rows(img)
    stream = zlib_stream(lines, img.shape[1] + 1, C, stats)
    if cap is not None and len(stream) > cap:
        return b"", ST_FULL, img, lines
    return stream, ST_OK, img, lines


# ------------------------------------------------------------------------------------------------ the cases the block layer adds

FIB = [1, 1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 233, 377, 610, 987, 1597, 2584, 4181, 6765, 10946, 17711]


def checker_rows(values, height, width, seed):
    """rows of byte magnitudes drawn from `values` (a list with repeats: the distribution), + on the cells of one colour of a checkerboard
    and - on the other: the None filter wins every row, no two neighbours are equal, and no byte equals the one above it"""
    g = R._rng(seed)
    mag = g.permutation(np.resize(np.asarray(values, np.int64), height * width)).reshape(height, width)
    yy, xx = np.mgrid[0:height, 0:width]
    return np.where((yy + xx) % 2 == 0, mag, 256 - mag).astype(np.int64)


def fibonacci_map(width=16384, height=5, seed=50, plant=(1, 9000, 200)):
    """literals with Fibonacci counts in every block (magnitudes 1..22, the k-th with weight FIB[k]: an unrestricted depth past 15), and
    one planted row match: `plant` = (row, column, length) copies that stretch of the row above"""
    values = []
    for k, f in enumerate(reversed(FIB)):
        values += [k + 1] * f
    m = checker_rows(values, height, width, seed)
    if plant is not None:
        y, x, n = plant
        m[y, x:x + n] = m[y - 1, x:x + n]
    return m


def sprinkled_row(width, extras, seed):
    """one row of +-1 / +-2 noise (None wins) with the byte values `extras` written once each, apart from one another"""
    row = R.signed_noise(width, seed)
    step = (width - 8) // max(len(extras), 1)
    assert step >= 2
    for k, v in enumerate(extras):
        row[4 + k * step] = v
    return row[None]


def header_row(C):
    """used literal symbols chosen for the run-length rule: zero runs of 139 (2 .. 142), 3, 10 and 11 between single-count symbols, and
    groups of 4 and 7 neighbouring single-count symbols (equal lengths: a repeat of 3 and of 6)"""
    extras = [142, 146, 157, 169] + list(range(175, 179)) + list(range(185, 192)) + list(range(200, 210))
    return sprinkled_row(C - 1, extras, 60)


def dyn_cases(C):
    """-> list of (name, int64 map, out_hw or None): what the block layer needs beyond png_enc_ref.cases"""
    out = [("zero1x1", np.zeros((1, 1), np.int64), None)]
    out.append(("chunks1", R.label_like(4, C // 4 - 1, 31), None))              # exactly C raw bytes
    out.append(("chunks16", R.label_like(64, 1000, 32), None))
    out.append(("chunks17", R.label_like(66, 1000, 33), None))                  # a one-chunk last block of 530 bytes
    out.append(("chunks33", R.label_like(100, 1330, 34), None))
    out.append(("noise17", R._rng(35).integers(0, 144, size=(2, 8 * C + 20)).astype(np.int64), None))   # S > 32768, a last block of 42 bytes
    out.append(("header_runs", header_row(C), None))
    out.append(("cl_limit", cl_limit_row(), None))
    out.append(("fibonacci", fibonacci_map(), None))
    out.append(("bigS", R.rows_repeat(32768, 36, height=3), None))
    out.append(("label512up", R.label_like(64, 128, 37), (200, 401)))
    return out


# magnitude -> exponent: the byte values v and 256 - v occur 2^e times each.  Found by a random search for literal counts whose code
# lengths make the code-length symbols themselves skewed enough for an unrestricted depth of 8
CL_LIMIT_EXPS = {40: 5, 41: 4, 28: 2, 11: 4, 59: 8, 51: 2, 25: 5, 15: 4, 43: 8, 14: 5, 31: 1, 26: 5, 6: 0, 60: 4, 46: 4, 56: 4, 13: 4, 37: 8,
                 32: 8, 55: 8, 4: 4, 39: 5, 23: 1, 3: 10, 44: 8, 30: 10, 58: 0, 19: 4, 53: 8, 52: 10, 63: 10, 2: 8, 9: 8, 18: 4, 20: 2,
                 42: 6, 38: 8, 61: 5, 49: 5, 5: 5, 62: 4, 16: 8, 47: 4, 57: 8, 33: 0, 12: 4, 54: 5, 35: 4, 17: 8, 50: 4, 21: 8, 27: 2,
                 7: 4, 48: 2, 1: 1}


def cl_limit_row():
    """one row, + magnitudes on even columns and - on odd ones (None wins, no runs), every magnitude 2^e times on either side"""
    mags = np.concatenate([np.full(1 << e, v, np.int64) for v, e in sorted(CL_LIMIT_EXPS.items())])
    row = np.empty(2 * len(mags), np.int64)
    row[0::2] = R._rng(61).permutation(mags)
    row[1::2] = 256 - R._rng(62).permutation(mags)
    return row[None]


def all_cases(C):
    return R.cases(C) + dyn_cases(C)


_ENCODED = {}


def encoded_cases(C):
    """the whole matrix through encode(), once per chunk size: (list of (name, map, out_hw, stream, status, resized map, scanlines), stats)"""
    if C not in _ENCODED:
        stats = new_stats()
        rows = []
        for name, m, out_hw in all_cases(C):
            stream, status, img, lines = encode(m, out_hw, C, stats=stats)
            rows.append((name, m, out_hw, stream, status, img, lines))
        _ENCODED[C] = (rows, stats)
    return _ENCODED[C]
