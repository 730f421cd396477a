"""TEST REFERENCE (not part of the product package): the lane line-IoU location loss of csrc/hn_lane_liou.hip (CLRNet, CVPR
2022, section 3.4) restated in float64 numpy, an fp32 restatement in the kernels' summation order, and the seeded inputs that
tests/test_lane_liou_cpu.py (which pins these functions) and tests/test_lane_liou_gpu.py (which holds the kernels to them) share.

Layout: rows of L = 2 P + 2 columns; [0, P) the x-offsets of the down part, P and P + 1 the two lengths, [P + 2, 2 P + 2) the x-offsets of
the up part; a column is valid iff target != 0."""
import numpy as np

F64 = np.float64


def x_columns(P):
    """bool [2 P + 2]: the x-offset columns"""
    m = np.ones(2 * P + 2, bool)
    m[P] = m[P + 1] = False
    return m


def lane_liou(pred, target, pmask, posn, P, e, alpha=10.0, gout=1.0):
    """float64.  pred / target [M, 2 P + 2], pmask bool [M], posn = max(#pos, 1) ->
    (loss, pos_liou, dpred [M, L], I [M], U [M], nrm [M]); I = U = 0 on rows that are not positive.
    Per positive row with X = valid x-columns, n = |X|, d = |p - t|: I = sum_X (2e - d), U = sum_X (2e + d), term 1 - I / U (0 when n = 0),
    plus sum over the valid length columns of alpha huber(p - t) / nrm, nrm = max(#valid columns of the row, 1);
    loss = sum over the positive rows / posn; pos_liou = mean I / U over the positive rows with n > 0 (0 without one)."""
    p, t = np.asarray(pred, F64), np.asarray(target, F64)
    M, L = p.shape
    assert L == 2 * P + 2 and e > 0
    pm = np.asarray(pmask, bool)
    xc = x_columns(P)
    valid = t != 0
    vx = valid & xc[None, :] & pm[:, None]
    vl = valid & ~xc[None, :] & pm[:, None]
    nrm = np.maximum(valid.sum(1), 1).astype(F64)
    diff = p - t
    d = np.abs(diff)
    n = vx.sum(1).astype(F64)
    S = (d * vx).sum(1)
    I, U = 2 * e * n - S, 2 * e * n + S
    has = n > 0
    liou = np.where(has, I / np.where(has, U, 1.0), 0.0)
    row = np.where(has, 1.0 - liou, 0.0)
    hub = np.where(d < 1, diff * diff / 2, d - 0.5)
    length = (alpha * hub * vl).sum(1) / nrm
    loss = (row + length).sum() / posn
    pos_liou = liou[has].sum() / max(int(has.sum()), 1)
    gx = np.where(has, 4 * e * n / np.where(has, U, 1.0) ** 2, 0.0)
    dh = np.where(d < 1, diff, np.sign(diff))
    grad = (np.sign(diff) * vx * gx[:, None] + dh * vl * alpha / nrm[:, None]) / posn * gout
    return float(loss), float(pos_liou), grad, I, U, nrm


def lane_liou_direct(pred, target, pmask, posn, P, e, alpha=10.0):
    """the same loss from the segments themselves, point by point: every valid x-column is the pair of segments [p - e, p + e] and
    [t - e, t + e]; overlap min(p + e, t + e) - max(p - e, t - e) (negative when they are disjoint) over hull max(..) - min(..), both
    summed over the row before the division -> (loss, pos_liou)"""
    p, t = np.asarray(pred, F64), np.asarray(target, F64)
    M, L = p.shape
    total, lious = 0.0, []
    for r in range(M):
        if not pmask[r]:
            continue
        cnt = int((t[r] != 0).sum())
        inter = union = 0.0
        n = 0
        for c in list(range(P)) + list(range(P + 2, L)):
            if t[r, c] != 0:
                inter += min(p[r, c] + e, t[r, c] + e) - max(p[r, c] - e, t[r, c] - e)
                union += max(p[r, c] + e, t[r, c] + e) - min(p[r, c] - e, t[r, c] - e)
                n += 1
        if n:
            lious.append(inter / union)
            total += 1.0 - inter / union
        for c in (P, P + 1):
            if t[r, c] != 0:
                dd = p[r, c] - t[r, c]
                total += alpha * (dd * dd / 2 if abs(dd) < 1 else abs(dd) - 0.5) / max(cnt, 1)
    return total / posn, (sum(lious) / len(lious) if lious else 0.0)


def _block_sum_1024_f32(v):
    """fp32 sum of 1024 per-thread values in the order of the finalize kernel: inside every 16-lane row four rotate-and-add steps (by 8, 4,
    2, 1), the four rows of a wave as (r0 + r1) + (r2 + r3), then the sixteen waves left to right"""
    f = np.float32
    v = np.asarray(v, f).reshape(16, 4, 16).copy()
    for k in (8, 4, 2, 1):
        v = (v + np.roll(v, k, axis=2)).astype(f)
    w = v[:, :, 0]
    waves = ((w[:, 0] + w[:, 1]).astype(f) + (w[:, 2] + w[:, 3]).astype(f)).astype(f)
    tot = f(0)
    for x in waves:
        tot = f(tot + x)
    return tot


def _tree32_f32(v):
    """[rows, 32] fp32 lane partials -> lane 0 of the xor tree from offset 16 down"""
    v = np.asarray(v, np.float32).copy()
    idx = np.arange(32)
    for o in (16, 8, 4, 2, 1):
        v = (v + v[:, idx ^ o]).astype(np.float32)
    return v[:, 0]


def lane_liou_f32(pred, target, pmask, posn, P, e, alpha=10.0, gout=1.0):
    """lane_liou in fp32 with the kernels' association: column c goes to lane c % 32, lanes add their columns in ascending order, a xor
    tree joins the lanes; the finalize adds rows i, i + 1024, ... per thread and then _block_sum_1024_f32 -> (loss, pos_liou, dpred)
    as fp32.  (The compiler may fuse a product into the following sum; that is at most one rounding less per operation.)"""
    f = np.float32
    p, t = np.asarray(pred, f), np.asarray(target, f)
    M, L = p.shape
    pm = np.asarray(pmask, bool)
    e, alpha, posn, gout = f(e), f(alpha), f(posn), f(gout)
    sd, n, cnt, sl = (np.zeros((M, 32), f) for _ in range(4))
    for c in range(L):
        ln = c % 32
        v = t[:, c] != 0
        cnt[:, ln] = cnt[:, ln] + v.astype(f)
        act = v & pm
        diff = (p[:, c] - t[:, c]).astype(f)
        ad = np.abs(diff)
        if c in (P, P + 1):
            hub = np.where(ad < 1, (f(0.5) * diff).astype(f) * diff, ad - f(0.5)).astype(f)
            sl[:, ln] = (sl[:, ln] + np.where(act, (hub * alpha).astype(f), f(0))).astype(f)
        else:
            sd[:, ln] = (sd[:, ln] + np.where(act, ad, f(0))).astype(f)
            n[:, ln] = n[:, ln] + act.astype(f)
    sd, n, cnt, sl = (_tree32_f32(v) for v in (sd, n, cnt, sl))
    nrm = np.maximum(cnt, f(1))
    w = ((f(2) * e) * n).astype(f)
    I, U = (w - sd).astype(f), (w + sd).astype(f)
    has = n > 0
    safe = np.where(has, U, f(1))
    rowloss = (np.where(has, ((f(2) * sd).astype(f) / safe).astype(f), f(0)) + (sl / nrm).astype(f)).astype(f)
    liou = np.where(U > 0, (I / np.where(U > 0, U, f(1))).astype(f), f(0)).astype(f)
    s, q, k = (np.zeros(1024, f) for _ in range(3))
    for i in range(M):
        th = i % 1024
        s[th] = f(s[th] + rowloss[i])
        if U[i] > 0:
            q[th] = f(q[th] + liou[i])
            k[th] = f(k[th] + f(1))
    loss = f(_block_sum_1024_f32(s) / posn)
    pos_liou = f(_block_sum_1024_f32(q) / max(_block_sum_1024_f32(k), f(1)))
    nl = (t[:, P] != 0).astype(f) + (t[:, P + 1] != 0).astype(f)
    nb = (nrm - nl).astype(f)
    gx = np.where(U > 0, ((((f(4) * e) * nb).astype(f) / (safe * safe).astype(f)).astype(f) / posn).astype(f) * gout, f(0)).astype(f)
    grad = np.zeros((M, L), f)
    for c in range(L):
        act = (t[:, c] != 0) & pm
        diff = (p[:, c] - t[:, c]).astype(f)
        if c in (P, P + 1):
            dh = np.where(np.abs(diff) < 1, diff, np.sign(diff)).astype(f)
            g = ((((dh * alpha).astype(f) / nrm).astype(f) / posn).astype(f) * gout).astype(f)
        else:
            g = (np.sign(diff).astype(f) * gx).astype(f)
        grad[:, c] = np.where(act, g, f(0))
    return loss, pos_liou, grad


FAR = 9.0       # |pred - target| on the row whose segments are disjoint everywhere: above 2 e for every half width e <= 4 the tests use


def lane_liou_case(P, M, seed):
    """inputs of the line-IoU tests (fp32 values), M >= 16 rows of 2 P + 2 columns -> (pred, target, pmask bool [M], posn).
    x targets on a 1/8 grid in [-5, 5] with ~30 % zeros (invalid points), length targets whole numbers in [0, P]; predictions are the
    targets plus noise of standard deviation 1.5, so the lengths' Huber argument falls on both sides of 1.  In every case:
      row 0   positive, down-part points only (and only the down length)       row 1   positive, up-part points only
      row 2   positive, every column valid                                      row 3   positive, no valid x-column, both lengths valid
      row 4   positive, every x prediction equals its target: liou = 1, zero x gradient
      row 5   positive, |pred - target| >= FAR at every x: liou < 0
      row 6   positive, 1e-6 targets (the encoder's stand-in for a true zero offset) among its x-columns
      row 7   negative, every column valid, predictions far off: its gradient must be 0
      row 8   positive, not a single valid column (normaliser clamps to 1)
      row 9   positive, predictions uniform in [-50, 50], lengths included
    the other rows are positive with probability 0.4; negatives carry non-zero targets and predictions like everyone else."""
    assert M >= 16 and P >= 1
    L = 2 * P + 2
    g = np.random.default_rng(1000 * seed + 10 * P + M)
    xc = x_columns(P)
    t = (g.integers(-40, 41, (M, L)) / 8.0) * (g.random((M, L)) < 0.7)
    t[:, P] = g.integers(0, P + 1, M)
    t[:, P + 1] = g.integers(0, P + 1, M)
    dense = np.where(g.random((M, L)) < 0.5, 1, -1) * (g.integers(1, 41, (M, L)) / 8.0)       # no zeros
    dense[:, ~xc] = g.integers(1, P + 1, (M, 2))
    down, up = np.arange(L) < P, np.arange(L) >= P + 2
    for r in (0, 1, 2, 3, 4, 5, 6, 7, 9):
        t[r] = dense[r]
    t[0, up] = 0.0
    t[0, P + 1] = 0.0
    t[1, down] = 0.0
    t[1, P] = 0.0
    t[3, xc] = 0.0
    t[6, 0] = 1e-6
    t[6, L - 1] = 1e-6
    t[8] = 0.0
    t = t.astype(np.float32)
    p = (t + g.standard_normal((M, L)) * 1.5).astype(np.float32)
    p[4, xc] = t[4, xc]
    far = (t[5] + np.where(g.random(L) < 0.5, 1, -1) * (FAR + g.random(L) * 4)).astype(np.float32)
    p[5, xc] = far[xc]
    p[7] = (t[7] + 20.0).astype(np.float32)
    p[9] = g.uniform(-50, 50, L).astype(np.float32)
    pmask = g.random(M) < 0.4
    pmask[[0, 1, 2, 3, 4, 5, 6, 8, 9]] = True
    pmask[7] = False
    return p, t, pmask, float(max(int(pmask.sum()), 1))
