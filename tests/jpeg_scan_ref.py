"""The device's JPEG scan decode (multitask_hydranet_amd/csrc/hn_jpeg_scan.hip) restated in Python / numpy in its PARALLEL
formulation: subsequences of S raw bytes, windows of T subsequences decoded from guessed states and again, round after round, from their
predecessors' exit states until no state changes, the block-count scan, the write pass from the exact entry states with DC differences, and
the segmented DC sum.  The state transitions are the kernels', decision for decision; every index formed is asserted to be in range.

    coefs, status, rounds = decode(data, head, scan_record, S)      # rounds: per window, the rounds in which a subsequence was decoded
    coefs, status = decode_serial(data, head, scan_record)          # one decoder over the whole scan with the record's tables
"""
import numpy as np

T = 256                                 # JPEG_SCAN_WINDOW
DONE = 0xFFFFFFFF
NATURAL = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56,
           57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]
M64 = (1 << 64) - 1
OK, NOBITS, BAD = 0, 1, 2


class Geom:
    def __init__(self, rec):
        r = rec[0] if rec.ndim else rec
        self.ncomp, self.hs, self.vs, self.mcus_x, self.mcus_y = (int(r[k]) for k in ("ncomp", "hs", "vs", "mcus_x", "mcus_y"))
        self.hv = self.hs * self.vs
        self.bpm = self.hv + 2 if self.ncomp == 3 else 1
        self.bw, self.start, n = [], [], 0
        for c in range(self.ncomp):
            self.bw.append(self.mcus_x * (1 if c else self.hs))
            self.start.append(n)
            n += self.bw[c] * self.mcus_y * (1 if c else self.vs)
        self.nblocks = n
        self.ri = int(r["restart_interval"])
        self.ib = self.ri * self.bpm
        self.td, self.ta = [int(v) for v in r["td"]], [int(v) for v in r["ta"]]
        tab = lambda t: dict(look_n=t["look_n"].tolist(), look_v=t["look_v"].tolist(), maxcode=t["maxcode"].tolist(),
                             valoff=t["valoff"].tolist(), vals=t["vals"].tolist())
        self.dc, self.ac = [tab(r["dc"][k]) for k in range(3)], [tab(r["ac"][k]) for k in range(3)]

    def place(self, blk):
        """scan-order block number -> block index in the coefficient buffer"""
        assert 0 <= blk < self.nblocks
        mcu, mm = divmod(blk, self.bpm)
        my, mx = divmod(mcu, self.mcus_x)
        c = 0 if mm < self.hv else mm - self.hv + 1
        v, u = divmod(mm, self.hs) if c == 0 else (0, 0)
        dest = self.start[c] + (my * (1 if c else self.vs) + v) * self.bw[c] + mx * (1 if c else self.hs) + u
        assert 0 <= dest < self.nblocks
        return dest


class Reader:
    """MSB-first bits of the scan, FF 00 un-stuffed in line; bitpos() is canonical: (raw byte, bit), never on a stuffed 00"""

    def __init__(self, scan):
        self.p, self.n = scan, len(scan)
        self.pos = self.acc = self.avail = self.ff = 0
        self.stop = False

    def byte(self, i):
        assert 0 <= i < self.n, (i, self.n)
        return self.p[i]

    def seek(self, bitpos):
        self.pos, self.acc, self.avail, self.ff, self.stop = bitpos >> 3, 0, 0, 0, False
        if bitpos & 7:
            self.fill()
            self.take(bitpos & 7)

    def fill(self):
        while self.avail <= 56 and not self.stop:
            if self.pos >= self.n:
                self.stop = True
                break
            b = self.byte(self.pos)
            if b == 0xFF:
                if self.pos + 1 >= self.n or self.byte(self.pos + 1) != 0:
                    self.stop = True
                    break
                self.pos += 2
                self.ff = ((self.ff << 1) | 1) & 0xFFFFFFFF
            else:
                self.pos += 1
                self.ff = (self.ff << 1) & 0xFFFFFFFF
            self.acc |= b << (56 - self.avail)
            self.avail += 8

    def take(self, k):
        if k > self.avail:
            return False
        self.acc = (self.acc << k) & M64
        self.avail -= k
        return True

    def bitpos(self):
        cnt = (self.avail + 7) >> 3
        raw = self.pos - cnt - bin(self.ff & ((1 << cnt) - 1)).count("1")
        return raw * 8 + ((-self.avail) & 7)


def decode_sym(rd, t):
    if rd.avail < 16:
        rd.fill()
    idx = rd.acc >> 55
    ln = t["look_n"][idx]
    if ln:
        return (OK if rd.take(ln) else NOBITS), t["look_v"][idx]
    for ln in range(10, 17):
        code = rd.acc >> (64 - ln)
        if code <= t["maxcode"][ln]:
            sym = t["vals"][(code + t["valoff"][ln]) & 255]
            return (OK if rd.take(ln) else NOBITS), sym
    if rd.avail < 16:
        return NOBITS, 0
    rd.take(16)
    return BAD, 0


def receive_extend(rd, sbits):
    if rd.avail < sbits:
        rd.fill()
    raw = rd.acc >> (64 - sbits)
    if not rd.take(sbits):
        return None
    return raw - (1 << sbits) + 1 if raw < (1 << (sbits - 1)) else raw


def decode_subseq(rd, g, st, end_bit, blk=None, out=None):
    """the symbols that start in [st.pos, end_bit) from state st = (bit position, m, z) -> (exit state, blocks completed, error seen).
    With `out` the state is exact, `blk` is the number of the block it is in, coefficients are written and the error counts."""
    pos, m, z = st
    if pos >= end_bit:
        return st, 0, False
    write = out is not None
    rd.seek(pos)
    completed, err = 0, False
    while True:
        sp = rd.bitpos()
        if sp >= end_bit:
            pos = sp
            break
        if write and blk >= g.nblocks:
            pos = DONE
            break
        dest = g.place(blk) if write else -1
        comp = 0 if m < g.hv else m - g.hv + 1
        assert 0 <= comp < g.ncomp and 0 <= z < 64
        block_end = nobits = False
        if z == 0:
            rc, s = decode_sym(rd, g.dc[g.td[comp]])
            if rc == NOBITS:
                nobits = True
            elif rc == BAD or s > 15:
                err = block_end = True
            else:
                diff = receive_extend(rd, s) if s else 0
                if diff is None:
                    nobits = True
                else:
                    if write:
                        out[dest, 0] = diff
                    z = 1
        else:
            rc, rs = decode_sym(rd, g.ac[g.ta[comp]])
            if rc == NOBITS:
                nobits = True
            elif rc == BAD:
                err = block_end = True
            else:
                run, sz = rs >> 4, rs & 15
                if sz:
                    k = z + run
                    if k > 63:
                        err = block_end = True
                    else:
                        v = receive_extend(rd, sz)
                        if v is None:
                            nobits = True
                        else:
                            if write:
                                out[dest, NATURAL[k]] = v
                            z = k + 1
                            block_end = z > 63
                elif run == 15:
                    z += 16
                    block_end = z > 63
                else:
                    block_end = True
        if nobits:
            i = rd.pos
            while i + 1 < rd.n and rd.byte(i) == 0xFF and rd.byte(i + 1) == 0xFF:
                i += 1
            mk = rd.byte(i + 1) if i + 1 < rd.n and rd.byte(i) == 0xFF else 0
            if mk < 0xD0 or mk > 0xD7:
                err, pos = True, DONE
                break
            if write:
                iv = blk // g.ib if g.ib else 0
                if not (g.ib and z == 0 and m == 0 and rd.avail < 8 and blk > 0 and iv * g.ib == blk and ((iv - 1) & 7) == mk - 0xD0):
                    err = True
            m = z = 0
            rd.seek((i + 2) * 8)
            continue
        if block_end:
            completed += 1
            m = 0 if m + 1 == g.bpm else m + 1
            z = 0
            if write:
                blk += 1
                if g.ib and blk < g.nblocks and blk % g.ib == 0:
                    bp = rd.bitpos()
                    i = bp >> 3
                    if bp & 7:
                        i += 2 if rd.byte(i) == 0xFF else 1
                    while i + 1 < rd.n and rd.byte(i) == 0xFF and rd.byte(i + 1) == 0xFF:
                        i += 1
                    if not (i + 1 < rd.n and rd.byte(i) == 0xFF and (rd.byte(i + 1) & 0xF8) == 0xD0):
                        err = True
    return (pos, m, z), completed, err


def dc_sums(g, out):
    """per component: the inclusive sum of the DC differences in scan order, restarted at every restart interval, wrapped to int16"""
    for c in range(g.ncomp):
        per, ch, cv = (g.hv, g.hs, g.vs) if c == 0 else (1, 1, 1)
        j = np.arange(g.mcus_x * g.mcus_y * per)
        mcu, q = j // per, j % per
        v, u = q // ch, q % ch
        my, mx = mcu // g.mcus_x, mcu % g.mcus_x
        idx = g.start[c] + (my * cv + v) * g.bw[c] + mx * ch + u
        assert idx.min() >= 0 and idx.max() < g.nblocks and len(np.unique(idx)) == len(idx)
        d = out[idx, 0].astype(np.int64)
        seg = g.ri * per if g.ri else len(j)
        pad = (-len(d)) % seg
        s = np.cumsum(np.concatenate([d, np.zeros(pad, np.int64)]).reshape(-1, seg), axis=1).reshape(-1)[:len(d)]
        out[idx, 0] = (s & 0xFFFF).astype(np.uint16).view(np.int16)


def _scan(data, rec):
    r = rec[0] if rec.ndim else rec
    o, n = int(r["scan_offset"]), int(r["scan_bytes"])
    assert 0 <= o and n > 0 and o + n <= len(data)
    return list(bytes(data[o:o + n]))


def decode_serial(data, head, rec):
    g = Geom(rec)
    assert g.nblocks * 128 == head["coef_bytes"]
    scan = _scan(data, rec)
    out = np.zeros((g.nblocks, 64), dtype=np.int16)
    _, done, err = decode_subseq(Reader(scan), g, (0, 0, 0), len(scan) * 8, 0, out)
    dc_sums(g, out)
    return out, int(err or done < g.nblocks)


def straddles(data, rec, S):
    """which boundary cases the scan holds at subsequence size S: an FF 00 pair and an RSTn marker with a subsequence boundary between
    their two bytes, fewer bytes than one subsequence, more than one window"""
    scan = _scan(data, rec)
    n = len(scan)
    at = [b for b in range(S, n, S) if scan[b - 1] == 0xFF]
    return {"ff00": any(scan[b] == 0 for b in at), "rst": any(0xD0 <= scan[b] <= 0xD7 for b in at), "short": n < S, "windows": n > S * T}


def decode(data, head, rec, S):
    g = Geom(rec)
    assert g.nblocks * 128 == head["coef_bytes"]
    scan = _scan(data, rec)
    n = len(scan)
    rd = Reader(scan)
    nsub = (n + S - 1) // S
    entries, rounds = [], []
    carry, blockbase = (0, 0, 0), 0
    for w0 in range(0, nsub, T):
        cnt_t = min(T, nsub - w0)
        ends = [min((w0 + t + 1) * S, n) * 8 for t in range(cnt_t)]
        ins = []
        for t in range(cnt_t):
            if t == 0:
                ins.append(carry)
            else:
                b = (w0 + t) * S
                if rd.byte(b - 1) == 0xFF:
                    b += 1
                ins.append((b * 8, 0, 0))
        res = [decode_subseq(rd, g, ins[t], ends[t]) for t in range(cnt_t)]
        nround = 1
        while True:
            prev = [carry] + [res[t][0] for t in range(cnt_t - 1)]           # every thread reads before any thread writes
            changed = [t for t in range(cnt_t) if prev[t] != ins[t]]
            if not changed:
                break
            nround += 1
            assert nround <= T + 1
            for t in changed:
                ins[t] = prev[t]
                res[t] = decode_subseq(rd, g, ins[t], ends[t])
        rounds.append(nround)
        for t in range(cnt_t):
            entries.append((ins[t], blockbase))
            blockbase += res[t][1]
        carry = res[cnt_t - 1][0]
    status = int(blockbase < g.nblocks)
    out = np.zeros((g.nblocks, 64), dtype=np.int16)
    for i, (st, first) in enumerate(entries):
        _, _, err = decode_subseq(rd, g, st, min((i + 1) * S, n) * 8, first, out)
        status |= int(err)
    dc_sums(g, out)
    return out, status, rounds
