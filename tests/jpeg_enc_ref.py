"""The device stage of the JPEG encode (multitask_hydranet_amd/jpeg_encode.py) restated in integer numpy from its
specification -- libjpeg's default compressor: quality-scaled Annex K tables, the 16-bit fixed-point RGB -> YCbCr tables, h2v1 / h2v2
down-sampling with alternating bias, edge replication (right to whole MCUs; down to a whole row group, then the DOWN-SAMPLED rows to the
MCU height), the accurate integer forward DCT on samples - 128 (tests/jpeg_ref.py's twelve 13-bit constants), quantisation by q * 8 with
round-half-up on magnitudes -- into the coefficient layout of jpeg.entropy_decode.  Blocks that exist only to fill an MCU (beyond the
component's own width / height in blocks) are zero here and on the device; the host entropy stage synthesises them.  int64 throughout."""
import numpy as np

from tests.jpeg_ref import C

SAMPLING = {"4:4:4": (1, 1), "4:2:2": (2, 1), "4:2:0": (2, 2), "grey": (1, 1)}

# Annex K.1 / K.2 of ITU-T T.81, natural (row-major) order
BASE_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                      18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112,
                      100, 103, 99], dtype=np.int64)
BASE_CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99]
                       + [99] * 32, dtype=np.int64)


def quant_tables(quality):
    """jpeg_set_quality + jpeg_add_quant_table (baseline): [luma, chroma], natural order"""
    q = min(100, max(1, int(quality)))
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return [np.clip((base * scale + 50) // 100, 1, 255) for base in (BASE_LUMA, BASE_CHROMA)]


def _fix(v):
    return int(v * 65536 + 0.5)


def ycc(bgr):
    b, g, r = (bgr[..., i].astype(np.int64) for i in range(3))
    half, off = 32768, 128 << 16
    y = (_fix(0.29900) * r + _fix(0.58700) * g + _fix(0.11400) * b + half) >> 16
    cb = (-_fix(0.16874) * r - _fix(0.33126) * g + _fix(0.50000) * b + off + half - 1) >> 16
    cr = (_fix(0.50000) * r - _fix(0.41869) * g - _fix(0.08131) * b + off + half - 1) >> 16
    return y, cb, cr


def _pad(p, h, w):
    return np.pad(p, ((0, h - p.shape[0]), (0, w - p.shape[1])), mode="edge")


def _down(p, hs, vs):
    if hs == 1:
        return p
    w2 = p.shape[1] // 2
    par = np.arange(w2) & 1
    if vs == 1:
        return (p[:, 0::2] + p[:, 1::2] + par[None]) >> 1
    return (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + (1 + par)[None]) >> 2


def _fdct_pass(d, first):
    """8-point forward DCT along the last axis: the row pass (results scaled up by 2 bits) or the column pass (descaled by 15)"""
    t0, t7 = d[..., 0] + d[..., 7], d[..., 0] - d[..., 7]
    t1, t6 = d[..., 1] + d[..., 6], d[..., 1] - d[..., 6]
    t2, t5 = d[..., 2] + d[..., 5], d[..., 2] - d[..., 5]
    t3, t4 = d[..., 3] + d[..., 4], d[..., 3] - d[..., 4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    o = [None] * 8
    if first:
        o[0], o[4], sh = (t10 + t11) << 2, (t10 - t11) << 2, 11
    else:
        o[0], o[4], sh = (t10 + t11 + 2) >> 2, (t10 - t11 + 2) >> 2, 15
    ds = lambda x: (x + (1 << (sh - 1))) >> sh
    z1 = (t12 + t13) * C["c0_541"]
    o[2], o[6] = ds(z1 + t13 * C["c0_765"]), ds(z1 - t12 * C["c1_847"])
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * C["c1_175"]
    a4, a5, a6, a7 = t4 * C["c0_298"], t5 * C["c2_053"], t6 * C["c3_072"], t7 * C["c1_501"]
    z1, z2, z3, z4 = -z1 * C["c0_899"], -z2 * C["c2_562"], -z3 * C["c1_961"] + z5, -z4 * C["c0_390"] + z5
    o[7], o[5], o[3], o[1] = ds(a4 + z1 + z3), ds(a5 + z2 + z4), ds(a6 + z2 + z3), ds(a7 + z1 + z4)
    return np.stack(o, -1)


def fdct(blk):
    """[n, 8, 8] int64 samples - 128 -> [n, 8, 8] coefficients scaled by 8"""
    d = _fdct_pass(blk, True)
    return _fdct_pass(d.transpose(0, 2, 1), False).transpose(0, 2, 1)


def quantise(co, qt):
    q = (np.asarray(qt, dtype=np.int64).reshape(8, 8) * 8)[None]
    r = (np.abs(co) + (q >> 1)) // q
    return np.where(co < 0, -r, r)


def head_for(w, h, subsampling, quality):
    """the header dict (jpeg.parse's keys) of the stream the encoder writes for a w x h frame"""
    hs, vs = SAMPLING[subsampling]
    ncomp = 1 if subsampling == "grey" else 3
    mx, my = -(-w // (8 * hs)), -(-h // (8 * vs))
    t = quant_tables(quality)
    return {"width": w, "height": h, "ncomp": ncomp, "hs": hs, "vs": vs, "mcus_x": mx, "mcus_y": my, "restart_interval": 0,
            "coef_bytes": mx * my * (hs * vs + (2 if ncomp == 3 else 0)) * 128, "qt": np.stack([t[0], t[1], t[1]]).astype(np.uint16)}


def real_blocks(head, c):
    """(blocks per row, per column) of component c that are pixel-derived: its own width / height in blocks"""
    hs, vs = (1, 1) if c == 0 else (head["hs"], head["vs"])
    return -(-(-(-head["width"] // hs)) // 8), -(-(-(-head["height"] // vs)) // 8)


def encode_coefs(bgr, subsampling="4:2:0", quality=95):
    """BGR uint8 [H, W, 3] -> (head, int16 [blocks, 64]); "grey" encodes channel 0"""
    h, w = bgr.shape[:2]
    head = head_for(w, h, subsampling, quality)
    hs, vs, mx, my = head["hs"], head["vs"], head["mcus_x"], head["mcus_y"]
    comps = [bgr[..., 0].astype(np.int64)] if head["ncomp"] == 1 else list(ycc(bgr))
    out = []
    for c, p in enumerate(comps):
        if c == 0:
            pp = _pad(p, my * vs * 8, mx * hs * 8)
        else:
            pp = _pad(p, -(-h // vs) * vs, mx * hs * 8)           # rows only to a whole row group, columns to whole MCUs
            pp = _pad(_down(pp, hs, vs), my * 8, mx * 8)           # then the down-sampled rows are replicated
        bh, bw = pp.shape[0] // 8, pp.shape[1] // 8
        blk = pp.reshape(bh, 8, bw, 8).transpose(0, 2, 1, 3).reshape(-1, 8, 8)
        q = quantise(fdct(blk - 128), head["qt"][c]).reshape(bh, bw, 64)
        rw, rh = real_blocks(head, c)
        q[rh:] = 0
        q[:, rw:] = 0
        out.append(q.reshape(-1, 64))
    co = np.concatenate(out).astype(np.int16)
    assert co.nbytes == head["coef_bytes"]
    return head, co


def fill_padding(head, coefs):
    """what the host entropy stage makes of the padding blocks (libjpeg's compress_data): AC zero, DC of the preceding block of the MCU"""
    co = np.array(coefs, dtype=np.int16).reshape(-1, 64)
    hs, vs, mx, my = head["hs"], head["vs"], head["mcus_x"], head["mcus_y"]
    if head["ncomp"] == 1 or (hs == 1 and vs == 1):
        return co
    rw, rh = real_blocks(head, 0)
    y = co[:mx * hs * my * vs].reshape(my * vs, mx * hs, 64)
    for m_y in range(my):
        for m_x in range(mx):
            prev = None
            for v in range(vs):
                for u in range(hs):
                    by, bx = m_y * vs + v, m_x * hs + u
                    if by >= rh or bx >= rw:
                        y[by, bx] = 0
                        y[by, bx, 0] = prev
                    prev = y[by, bx, 0]
    return co
