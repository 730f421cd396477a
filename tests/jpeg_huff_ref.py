"""The device entropy stage of the JPEG encode (hn_jpeg_huff.hip) restated in numpy in its PARALLEL formulation, from the
specification (ITU-T T.81 F.1.2 with the Annex K.3 tables): every block's bit string is a function of that block and of the DC of one
earlier block whose index follows from the geometry alone; the strings are concatenated by a prefix sum of their lengths; the last byte is
padded with ones; the stuffed stream is a count of 0xFF bytes, a second prefix sum and a scatter.  No loop carries state from one block to
the next.  Blocks that only fill an MCU are not read: they are a DC difference of 0 and an end-of-block, and no block is predicted from
them.  A value no baseline table can code raises ValueError."""
import numpy as np

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49,
                   56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])
# Annex K.3: BITS (codes per length 1..16) and HUFFVAL of the typical tables, [luminance, chrominance]
DC_BITS = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], [0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0])
DC_VALS = list(range(12))
AC_BITS = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D], [0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77])
AC_VALS = (list(bytes.fromhex(
    "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a34353637"
    "38393a434445464748494a535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3"
    "a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa")), list(bytes.fromhex(
    "000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a3536"
    "3738393a434445464748494a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999a"
    "a2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa")))


def code_table(bits, vals):
    """Annex C: symbol -> (code, length) as two int64 [256] arrays (length 0: the symbol has no code)"""
    code, length = np.zeros(256, np.int64), np.zeros(256, np.int64)
    c, k = 0, 0
    for ln in range(1, 17):
        for _ in range(bits[ln - 1]):
            code[vals[k]], length[vals[k]] = c, ln
            c, k = c + 1, k + 1
        c <<= 1
    return code, length


DC = [code_table(DC_BITS[t], DC_VALS) for t in range(2)]
AC = [code_table(AC_BITS[t], AC_VALS[t]) for t in range(2)]


def bit_size(a):
    """bits of the magnitudes (0 for 0), element-wise"""
    a = np.asarray(a, dtype=np.int64)
    n = np.zeros(a.shape, np.int64)
    for k in range(16):
        n += (a >> k) > 0
    return n


def scan_blocks(head):
    """the scan's blocks in order (per MCU: Y in (v, u) order, Cb, Cr) -> component, is-real flag, index in the coefficient layout and
    index of the block it is predicted from (-1: predictor 0), each as an array over the scan.  Pure geometry."""
    hs, vs, mx_n, my_n, nc = head["hs"], head["vs"], head["mcus_x"], head["mcus_y"], head["ncomp"]
    w, h = head["width"], head["height"]
    ny = hs * vs
    bpm = ny + (2 if nc == 3 else 0)
    mcus = mx_n * my_n
    idx = np.arange(mcus * bpm, dtype=np.int64)
    m, j = idx // bpm, idx % bpm
    my, mx = m // mx_n, m % mx_n
    luma = j < ny
    comp = np.where(luma, 0, 1 + j - ny)
    bw0, rw0, rh0 = mx_n * hs, -(-w // 8), -(-h // 8)
    v, u = np.where(luma, j // hs, 0), np.where(luma, j % hs, 0)
    by, bx = my * vs + v, mx * hs + u
    real = ~luma | ((by < rh0) & (bx < rw0))
    start = [0, mcus * ny, mcus * ny + mcus]
    blk = np.where(luma, by * bw0 + bx, np.where(comp == 1, start[1], start[2]) + m)
    # the previous real block of the same component: chroma planes are 1 x 1 per MCU and have no filling blocks
    nu = lambda mxx: np.minimum(hs, rw0 - mxx * hs)                       # real luma blocks per row / column of an MCU
    nv = lambda myy: np.minimum(vs, rh0 - myy * vs)
    pmy, pmx = np.where(mx > 0, my, my - 1), np.where(mx > 0, mx - 1, mx_n - 1)
    prev_mcu_last = (pmy * vs + nv(pmy) - 1) * bw0 + pmx * hs + nu(pmx) - 1
    prev_luma = np.where(u > 0, blk - 1, np.where(v > 0, blk - bw0 + nu(mx) - 1, np.where(m > 0, prev_mcu_last, -1)))
    prev = np.where(luma, prev_luma, np.where(m > 0, blk - 1, -1))
    prev = np.where(real, prev, -1)
    return comp, real, blk, prev


def block_tokens(head, coefs):
    """-> (values, lengths) int64 [blocks of the scan, 65]: the DC code + difference, one slot per AC coefficient in zigzag order (its ZRL
    codes, its run/size code and its amplitude bits, or nothing for a zero), the end-of-block"""
    co = np.asarray(coefs).reshape(-1, 64).astype(np.int64)
    assert co.shape[0] * 128 == head["coef_bytes"]
    comp, real, blk, prev = scan_blocks(head)
    n = comp.size
    tab = (comp > 0).astype(np.int64)
    z = co[np.where(real, blk, 0)][:, ZIGZAG]                            # filling blocks: whatever is read is masked below
    pred = np.where(prev >= 0, co[np.maximum(prev, 0), 0], 0)
    val, length = np.zeros((n, 65), np.int64), np.zeros((n, 65), np.int64)
    dc_code, dc_len = np.stack([DC[0][0], DC[1][0]]), np.stack([DC[0][1], DC[1][1]])
    ac_code, ac_len = np.stack([AC[0][0], AC[1][0]]), np.stack([AC[0][1], AC[1][1]])
    amp = lambda x, s: np.where(x < 0, x - 1, x) & ((1 << s) - 1)
    diff = np.where(real, z[:, 0] - pred, 0)
    s = bit_size(np.abs(diff))
    if (s > 11).any():
        raise ValueError("a DC difference of more than 11 bits")
    val[:, 0] = (dc_code[tab, s] << s) | amp(diff, s)
    length[:, 0] = dc_len[tab, s] + s
    ac = np.where(real[:, None], z[:, 1:], 0)
    nz = ac != 0
    s = bit_size(np.abs(ac))
    if (s > 10).any():
        raise ValueError("an AC value of more than 10 bits")
    k = np.arange(1, 64)[None, :]
    last = np.maximum.accumulate(np.where(nz, k, 0), axis=1)             # position of the last non-zero up to and including k
    before = np.concatenate([np.zeros((n, 1), np.int64), last[:, :-1]], axis=1)
    run = k - before - 1                                                  # zeros between this coefficient and the previous non-zero one
    nzrl, sym = run >> 4, ((run & 15) << 4) | s
    t = tab[:, None]
    zc, zl = ac_code[t, 0xF0], ac_len[t, 0xF0]
    zrl_val = np.where(nzrl == 0, 0, np.where(nzrl == 1, zc, np.where(nzrl == 2, (zc << zl) | zc, (((zc << zl) | zc) << zl) | zc)))
    ln = ac_len[t, sym] + s
    assert (ac_len[t, sym][nz] > 0).all()
    val[:, 1:64] = np.where(nz, (zrl_val << ln) | (ac_code[t, sym] << s) | amp(ac, s), 0)
    length[:, 1:64] = np.where(nz, nzrl * zl + ln, 0)
    eob = last[:, -1] < 63
    val[:, 64] = np.where(eob, ac_code[tab, 0], 0)
    length[:, 64] = np.where(eob, ac_len[tab, 0], 0)
    return val, length


def concatenate(val, length):
    """tokens -> (the unstuffed stream as uint8, the last byte padded with ones; bits before the padding; bit offset of every block)"""
    v, ln = val.reshape(-1), length.reshape(-1)
    start = np.cumsum(ln) - ln                                           # exclusive prefix sum: where every token's bits land
    total = int(ln.sum())
    tok = np.repeat(np.arange(v.size), ln)
    j = np.arange(total) - start[tok]
    bits = ((v[tok] >> (ln[tok] - 1 - j)) & 1).astype(np.uint8)
    bits = np.concatenate([bits, np.ones((-total) % 8, np.uint8)])
    return np.packbits(bits), total, start.reshape(val.shape)[:, 0]


def stuff(stream):
    """a 0x00 after every 0xFF, by count and scatter"""
    ff = stream == 0xFF
    pos = np.arange(stream.size) + (np.cumsum(ff) - ff)                   # exclusive prefix sum of the counts
    out = np.zeros(stream.size + int(ff.sum()), np.uint8)
    out[pos] = stream
    return out


def scan_bytes(head, coefs):
    """the stuffed, one-padded scan of the image: what lies between the header and the EOI marker"""
    val, length = block_tokens(head, coefs)
    return stuff(concatenate(val, length)[0]).tobytes()
