"""The device stage of the JPEG decode (multitask_hydranet_amd/jpeg.py) restated in integer numpy from its specification --
libjpeg's default decode: dequantise, the accurate integer inverse DCT (13-bit constants, 2 extra bits after the column pass, descale,
+128, clamp), "fancy" triangle chroma up-sampling (plain replication when the chroma plane is at most 2 samples wide), the 16-bit
fixed-point YCbCr -> RGB conversion -- on the coefficient layout of jpeg.entropy_decode.  int64 throughout."""
import numpy as np

# round(x * 2**13) of the twelve rotation constants
C = dict(c0_298=2446, c0_390=3196, c0_541=4433, c0_765=6270, c0_899=7373, c1_175=9633, c1_501=12299, c1_847=15137, c1_961=16069, c2_053=16819,
         c2_562=20995, c3_072=25172)


def _idct_1d(d, shift):
    """8-point inverse DCT along axis 0 of d [8, ...] (int64), every output (sum + 2**(shift - 1)) >> shift"""
    z2, z3 = d[2], d[6]
    z1 = (z2 + z3) * C["c0_541"]
    t2 = z1 - z3 * C["c1_847"]
    t3 = z1 + z2 * C["c0_765"]
    t0 = (d[0] + d[4]) << 13
    t1 = (d[0] - d[4]) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    t0, t1, t2, t3 = d[7], d[5], d[3], d[1]
    z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
    z5 = (z3 + z4) * C["c1_175"]
    t0, t1, t2, t3 = t0 * C["c0_298"], t1 * C["c2_053"], t2 * C["c3_072"], t3 * C["c1_501"]
    z1, z2, z3, z4 = -z1 * C["c0_899"], -z2 * C["c2_562"], -z3 * C["c1_961"] + z5, -z4 * C["c0_390"] + z5
    t0, t1, t2, t3 = t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4
    r = 1 << (shift - 1)
    out = [t10 + t3, t11 + t2, t12 + t1, t13 + t0, t13 - t0, t12 - t1, t11 - t2, t10 - t3]
    return np.stack([(o + r) >> shift for o in out])


def idct_blocks(coefs, qt):
    """coefs int16 [n, 64] (natural order), qt [64] -> uint8 samples [n, 8, 8]"""
    d = (coefs.astype(np.int64) * qt.astype(np.int64)[None]).reshape(-1, 8, 8)
    ws = _idct_1d(d.transpose(1, 0, 2), 11)                       # columns: axis 0 = vertical frequency -> [row, n, column]
    px = _idct_1d(ws.transpose(2, 1, 0), 18)                      # rows: axis 0 = horizontal frequency -> [column, n, row]
    return np.clip(px.transpose(1, 2, 0) + 128, 0, 255).astype(np.uint8)


def planes(head, coefs):
    """the sample planes (padded to whole MCUs) of every component"""
    coefs = np.asarray(coefs).reshape(-1, 64)
    out, start = [], 0
    for c in range(head["ncomp"]):
        bw = head["mcus_x"] * (head["hs"] if c == 0 else 1)
        bh = head["mcus_y"] * (head["vs"] if c == 0 else 1)
        blk = idct_blocks(coefs[start:start + bw * bh], head["qt"][c])
        out.append(blk.reshape(bh, bw, 8, 8).transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8))
        start += bw * bh
    assert start == coefs.shape[0]
    return out


def _h2_fancy(p):
    """[h, cw] int64 -> [h, 2 cw]: (3 near + far + 1 or 2) >> 2, the two end columns copied"""
    left = np.concatenate([p[:, :1], p[:, :-1]], 1)
    right = np.concatenate([p[:, 1:], p[:, -1:]], 1)
    even, odd = (3 * p + left + 1) >> 2, (3 * p + right + 2) >> 2
    even[:, 0], odd[:, -1] = p[:, 0], p[:, -1]
    return np.stack([even, odd], 2).reshape(p.shape[0], -1)


def _h2v2_fancy(p):
    """[ch, cw] -> [2 ch, 2 cw]: column sums 3 near row + far row (edge rows replicated), then (3 this + neighbour + 8 or 7) >> 4"""
    up = np.concatenate([p[:1], p[:-1]], 0)
    down = np.concatenate([p[1:], p[-1:]], 0)
    rows = np.stack([3 * p + up, 3 * p + down], 1).reshape(-1, p.shape[1])        # output rows 2r (row above), 2r + 1 (row below)
    left = np.concatenate([rows[:, :1], rows[:, :-1]], 1)
    right = np.concatenate([rows[:, 1:], rows[:, -1:]], 1)
    even, odd = (3 * rows + left + 8) >> 4, (3 * rows + right + 7) >> 4
    even[:, 0], odd[:, -1] = (4 * rows[:, 0] + 8) >> 4, (4 * rows[:, -1] + 7) >> 4
    return np.stack([even, odd], 2).reshape(rows.shape[0], -1)


def upsample(plane, head):
    """a chroma plane -> int64 [H, W]"""
    W, H, hs, vs = head["width"], head["height"], head["hs"], head["vs"]
    cw, ch = -(-W // hs), -(-H // vs)
    p = plane[:ch, :cw].astype(np.int64)
    if hs == 2 and cw <= 2:
        p = np.repeat(np.repeat(p, vs, 0), 2, 1)
    elif hs == 2:
        p = _h2v2_fancy(p) if vs == 2 else _h2_fancy(p)
    return p[:H, :W]


def decode(head, coefs):
    """(header, quantised coefficients) -> BGR uint8 [H, W, 3]"""
    W, H = head["width"], head["height"]
    pl = planes(head, coefs)
    y = pl[0][:H, :W].astype(np.int64)
    if head["ncomp"] == 1:
        return np.repeat(y[..., None], 3, 2).astype(np.uint8)
    cb, cr = upsample(pl[1], head) - 128, upsample(pl[2], head) - 128
    fix = lambda v: int(v * 65536 + 0.5)
    r = y + ((fix(1.40200) * cr + 32768) >> 16)
    g = y + ((-fix(0.34414) * cb + 32768 - fix(0.71414) * cr) >> 16)
    b = y + ((fix(1.77200) * cb + 32768) >> 16)
    return np.clip(np.stack([b, g, r], 2), 0, 255).astype(np.uint8)
