"""Vectorised numpy restatements of the RAW outputs of the C entry points of csrc/hn_post.hip other than the detection NMS: lane decode +
lane NMS, input pre-processing, the seg confusion counts, the seg overlay, the lane rasteriser and the pair counts.  They restate the
kernels' index arithmetic, not the Python wrappers around them.  tests/test_post_ref_cpu.py holds every function here to the oracle's own
(loop-form) function on the cases of tests/post_cases.py; tests/test_post_exact_gpu.py holds the kernels to these with ==.

Every restatement takes `mutant=`: the name of ONE deliberately wrong variant of the restatement (never of a kernel).  The CPU test shows
that each mutant changes the expected output of at least one GPU case, i.e. that the suite would notice a kernel with that fault.

Float decisions follow the kernels' own float32 operations: every product, sum and quotient below is a numpy float32 operation rounded
on its own, in the kernels' order."""
import numpy as np
import torch

F32 = np.float32

MUTANTS = {
    "lane_decode_nms": ("tie_reversed", "thr_equal_dropped", "dis_strict", "down_walk_up_bound", "dead_suppresses"),
    "confusion": ("negative_to_class0",),
    "overlay": ("half_up", "sx1_unclamped"),
    "preprocess": ("sx1_unclamped",),
    "raster": ("zero_length_skipped", "radius_short"),
    "pair_counts": ("bit31_lost",),
}


def _mut(fn, mutant):
    assert mutant is None or mutant in MUTANTS[fn], (fn, mutant)
    return mutant


# =====================================================================================================================================
# lane decode + lane NMS
# =====================================================================================================================================
def lane_geometry(W, H, stride, ppl):
    """LaneGeo as hn_lane_decode_nms fills it (hn_post.hip, `g.fw = W / stride` ... `g.ppa = (double)ppl / g.fh`)"""
    fw, fh = W // stride, H // stride
    return dict(W=W, H=H, stride=stride, ppl=ppl, fw=fw, fh=fh, hw=fw * fh, L=2 * ppl + 2, interval=F32(H / ppl), ppa=ppl / fh)


def lane_lds_bytes(hw):
    """dynamic LDS of the launch (`lds = hw * 21 + 32`); above 64 KiB the entry point opts in, above hw = 7168 it refuses"""
    return hw * 21 + 32


def lane_softmax(cls):
    """prob of class 1, float32.  torch's softmax (what the oracle and the reference use); the kernel's expf form
    (`prob = __fdiv_rn(e1, __fadd_rn(e0, e1))`) agrees with it to the last place, and exactly on equal logits (0.5)"""
    return torch.softmax(torch.from_numpy(np.ascontiguousarray(cls, dtype=F32)), -1).numpy()[..., 1]


def _lead(ok):
    """length of the leading run of True along the last axis (a walk that `break`s at the first False)"""
    return np.cumprod(ok, axis=-1).sum(-1).astype(np.int32)


def lane_decode_nms(cls, loc, geometry, thr, nms_thr, use_mean, margin, mutant=None):
    """lane_decode_nms_kernel.  cls [N, hw, 2] logits, loc [N, hw, 2 ppl + 2] float32; geometry = (W, H, stride, ppl).
    Returns a dict: prob (float32), start, end (int32) [N, hw] for EVERY anchor (0, 0 below the threshold); X [N, hw, ppl] float32 with
    `written` [N, hw, ppl] marking start <= p < end (the kernel writes nothing else; X is NaN there); per image order[n], keep[n]
    (int32 arrays of count[n] entries) and count [N].

    first loop (`for (int a = tid; a < hw; a += 1024)`): threshold `!(prob < exist_thr)`, `ypos`, `cx`, the up walk (breaks on
    `(float)i >= rel_up || ypos + i >= g.ppl` and on `ax < 0.f || ax >= (float)g.W`), the down walk (`i < ypos`, `(float)i >= rel_down`,
    `ax >= (float)g.W + g.margin`), `valid = (end - start) >= 2`; second loop: the rank `s_prob[b] > prob || (s_prob[b] == prob && b < a)`
    over the valid anchors; third: the greedy walk, `hi <= lo || lo < 0 || hi < 1` skips a pair, the float32 running sum over lo <= i < hi,
    `__fdiv_rn(dis, (float)(hi - lo))`, the two end-point maxima unless use_mean, `dis <= nms_thr`."""
    m = _mut("lane_decode_nms", mutant)
    W, H, stride, ppl = geometry
    g = lane_geometry(W, H, stride, ppl)
    cls, loc = np.asarray(cls, F32), np.asarray(loc, F32)
    N, hw = cls.shape[:2]
    assert hw == g["hw"] and loc.shape == (N, hw, g["L"])
    thr32, nms32, margin32 = F32(thr), F32(nms_thr), F32(margin)
    prob = lane_softmax(cls)
    cand = ~(prob < thr32)
    if m == "thr_equal_dropped":
        cand = prob > thr32
    a = np.arange(hw)
    h, w = a // g["fw"], a % g["fw"]
    ypos = ((g["fh"] - 1 - h).astype(np.float64) * g["ppa"]).astype(np.int32)            # (int) of a non-negative double
    cx = ((1.0 * w + 0.5) * stride).astype(F32)
    i = np.arange(ppl)
    rel_down, rel_up = loc[:, :, ppl], loc[:, :, ppl + 1]
    ax_up = (cx[None, :, None] + loc[:, :, ppl + 2:] * g["interval"]).astype(F32)       # two float32 operations
    ax_dn = (cx[None, :, None] + loc[:, :, :ppl] * g["interval"]).astype(F32)
    with np.errstate(invalid="ignore"):
        ok_up = ~(i.astype(F32) >= rel_up[..., None]) & (ypos[None, :, None] + i < ppl) & ~((ax_up < 0) | (ax_up >= F32(W)))
        dn_bound = F32(W) if m == "down_walk_up_bound" else F32(F32(W) + margin32)
        ok_dn = (i < ypos[None, :, None]) & ~(i.astype(F32) >= rel_down[..., None]) & ~((ax_dn < 0) | (ax_dn >= dn_bound))
    n_up, n_dn = _lead(ok_up), _lead(ok_dn)
    start = np.where(cand, ypos[None] - n_dn, 0).astype(np.int32)
    end = np.where(cand, ypos[None] + n_up, 0).astype(np.int32)
    valid = cand & (end - start >= 2)
    X = np.full((N, hw, ppl), np.nan, F32)
    written = np.zeros((N, hw, ppl), bool)
    for k in range(ppl):                                                                # walk step k of both walks
        for ax, cnt, pos in ((ax_up, n_up, ypos[None] + k), (ax_dn, n_dn, ypos[None] - 1 - k)):
            nn, aa = np.nonzero(cand & (k < cnt))
            X[nn, aa, pos[0, aa]] = ax[nn, aa, k]
            written[nn, aa, pos[0, aa]] = True
    assert np.array_equal(written, (i >= start[..., None]) & (i < end[..., None]))
    order, keep = [], []
    for n in range(N):
        v = np.nonzero(valid[n])[0]
        # rank = #{b valid: prob_b > prob_a or (prob_b == prob_a and b < a)}: descending prob, raster order inside a tie
        o = v[np.lexsort((v if m != "tie_reversed" else -v, -prob[n, v].astype(np.float64)))].astype(np.int32)
        cnt = len(o)
        sup = np.zeros(cnt, bool)
        st, en, Xo = start[n, o], end[n, o], X[n, o]
        for k in range(cnt):
            if sup[k] and m != "dead_suppresses":
                continue
            t = np.arange(k + 1, cnt)
            lo, hi = np.maximum(st[k], st[t]), np.minimum(en[k], en[t])
            pair = ~((hi <= lo) | (lo < 0) | (hi < 1))
            t, lo, hi = t[pair], lo[pair], hi[pair]
            if not len(t):
                continue
            d = np.abs((Xo[k][None] - Xo[t]).astype(F32))                               # [pairs, ppl]; NaN outside either lane
            dis = np.zeros(len(t), F32)
            for p in range(ppl):
                inside = (p >= lo) & (p < hi)
                dis = np.where(inside, (dis + np.where(inside, d[:, p], 0)).astype(F32), dis)
            dis = (dis / (hi - lo).astype(F32)).astype(F32)
            if not use_mean:
                r = np.arange(len(t))
                dis = np.maximum(np.maximum(dis, d[r, lo]), d[r, hi - 1])
            hit = dis < nms32 if m == "dis_strict" else dis <= nms32
            sup[t[hit]] = True
        order.append(o)
        keep.append((~sup).astype(np.int32))
    return dict(prob=prob, start=start, end=end, X=X, written=written, order=order, keep=keep, count=np.array([len(o) for o in order], np.int32))


# =====================================================================================================================================
# the 8-bit bilinear resize shared by the pre-processing and the overlay
# =====================================================================================================================================
def lin_coef(dsize, ssize, mutant=None):
    """lin_coef of hn_post.hip for every destination index: (s0, s1, c0, c1).  `f = (float)((d + 0.5) * scale - 0.5)`, `s = floorf(f)`,
    `f -= s`, the two clamps (`s < 0`, `s >= ssize - 1`: f = 0), coefficients `__float2int_rn((1 - f) * 2048)`, `__float2int_rn(f * 2048)`;
    s1 is the callers' `sx + 1 < Ws ? sx + 1 : Ws - 1`."""
    scale = ssize / dsize
    f = ((np.arange(dsize, dtype=np.float64) + 0.5) * scale - 0.5).astype(F32)
    s = np.floor(f).astype(np.int32)
    f = (f - s.astype(F32)).astype(F32)
    lo, hi = s < 0, s >= ssize - 1
    f[lo], s[lo] = 0, 0
    f[hi], s[hi] = 0, ssize - 1
    c0 = np.rint((F32(1) - f) * F32(2048)).astype(np.int32)
    c1 = np.rint(f * F32(2048)).astype(np.int32)
    s1 = s + 1 if mutant == "sx1_unclamped" else np.minimum(s + 1, ssize - 1)
    return s, s1, c0, c1


def resize_u8(img, out_hw, mutant=None):
    """lin_bgr8 / the overlay's inline copy of it for uint8 [N, Hs, Ws, 3] -> [N, Hd, Wd, 3]: `h = r[sx] * ax0 + r[sx1] * ax1` on both
    rows, `(((by0 * (h0 >> 4)) >> 16) + ((by1 * (h1 >> 4)) >> 16) + 2) >> 2`, clamped to 0..255; an equal size is a copy.
    The `sx1_unclamped` mutant indexes column Ws: numpy raises IndexError where a kernel would read past the row (the coefficient of that
    column is 0 whenever the clamp acts, so no OUTPUT can show it; the out-of-range read itself is what the mutant stands for)."""
    n, hs, ws = img.shape[:3]
    hd, wd = out_hw
    if (hs, ws) == (hd, wd):
        return img.copy()
    sx0, sx1, ax0, ax1 = lin_coef(wd, ws, mutant)
    sy0, sy1, by0, by1 = lin_coef(hd, hs)
    src = img.astype(np.int32)
    hrow = src[:, :, sx0] * ax0[None, None, :, None] + src[:, :, sx1] * ax1[None, None, :, None]            # [n, hs, wd, 3]
    out = (((by0[None, :, None, None] * (hrow[:, sy0] >> 4)) >> 16) + ((by1[None, :, None, None] * (hrow[:, sy1] >> 4)) >> 16) + 2) >> 2
    return np.clip(out, 0, 255).astype(np.uint8)


def preprocess(frames_u8, out_hw, mutant=None):
    """preprocess_kernel: uint8 BGR [N, Hs, Ws, 3] -> float32 RGB [N, 3, Hd, Wd]; the resize above, then
    `q = ((double)v[2 - c] / 255.0 - mean[c]) / sd[c]`, `(float)q`"""
    m = _mut("preprocess", mutant)
    v = resize_u8(np.asarray(frames_u8, np.uint8), out_hw, m)[..., ::-1].astype(np.float64)
    q = (v / 255.0 - np.array([0.485, 0.456, 0.406])) / np.array([0.229, 0.224, 0.225])
    return np.ascontiguousarray(np.transpose(q, (0, 3, 1, 2))).astype(F32)


# =====================================================================================================================================
# seg confusion counts and overlay
# =====================================================================================================================================
def confusion(pred, target, C, mutant=None):
    """seg_confusion_kernel: int64 [(C + 1), (C + 1)], conf[p][t] = number of pixels with prediction p and target t after
    `p = (p > C || p < 0) ? C : p` (the same for t); a float32 target is `(long)` truncated toward zero first (4.99 -> 4, -0.5 -> 0)."""
    m = _mut("confusion", mutant)
    p = np.asarray(pred).astype(np.int64).reshape(-1)
    t = np.asarray(target)
    t = (np.trunc(t.astype(np.float64)) if t.dtype.kind == "f" else t).astype(np.int64).reshape(-1)

    def bucket(v):
        neg = 0 if m == "negative_to_class0" else C
        return np.where(v > C, C, np.where(v < 0, neg, v))
    idx = bucket(p) * (C + 1) + bucket(t)
    return np.bincount(idx, minlength=(C + 1) ** 2).astype(np.int64).reshape(C + 1, C + 1)


def overlay(mask, lut, frames, mutant=None):
    """seg_overlay_kernel: mask int64 [N, H, W], lut uint8 [ncls, 3], frames uint8 [N, Ho, Wo, 3] -> uint8 [N, Ho, Wo, 3].
    `colour`: `(k >= 0 && k < ncls) ? lut[k * 3 + c] : 0`; the resize above on the colours; the blend
    `__fadd_rn(__fmul_rn((float)f, 0.8f), __fmul_rn((float)v, 0.5f))`, `__float2int_rn` (half to even), saturation to 0..255."""
    m = _mut("overlay", mutant)
    mask, lut, frames = np.asarray(mask, np.int64), np.asarray(lut, np.uint8), np.asarray(frames, np.uint8)
    ncls = lut.shape[0]
    ok = (mask >= 0) & (mask < ncls)
    col = np.where(ok[..., None], lut[np.where(ok, mask, 0)], 0).astype(np.uint8)
    v = resize_u8(col, frames.shape[1:3], m if m == "sx1_unclamped" else None)
    s = ((frames.astype(F32) * F32(0.8)).astype(F32) + (v.astype(F32) * F32(0.5)).astype(F32)).astype(F32)
    r = np.floor(s.astype(np.float64) + 0.5) if m == "half_up" else np.rint(s)
    return np.clip(r, 0, 255).astype(np.uint8)


# =====================================================================================================================================
# lane rasteriser and pair counts
# =====================================================================================================================================
def raster(pts, seg_lane, seg_first, lane_width, H, W, n_lanes=None, mutant=None):
    """lane_raster_kernel: uint8 masks [n_lanes, H, W] (n_lanes defaults to the largest lane index + 1), 255 where a pixel lies within
    lane_width / 2 of one of the lane's segments.  Per segment: `r = (width2 + 3) / 4 + 1` with width2 = 2 lane_width, the bounding box
    clipped to the frame (`if (bx1 < bx0 || by1 < by0) return`), and the integer test `16 * num <= width2 * width2 * den` with
    num / den = the squared distance to the segment (`len2 == 0 || dot <= 0`: the first end point; `dot >= len2`: the second; else
    cross^2 / len2)."""
    m = _mut("raster", mutant)
    pts = np.asarray(pts, np.int64).reshape(-1, 2)
    n_lanes = n_lanes if n_lanes is not None else (int(np.max(seg_lane)) + 1 if len(seg_lane) else 0)
    masks = np.zeros((n_lanes, H, W), np.uint8)
    width2 = 2 * lane_width
    r = (width2 + 3) // 4 + 1
    if m == "radius_short":
        r -= 2                                            # (one less than (width2 + 3) / 4, the smallest radius that still covers)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.int64)
    for lane, i in zip(seg_lane, seg_first):
        (x0, y0), (x1, y1) = pts[i], pts[i + 1]
        bx0, bx1 = max(min(x0, x1) - r, 0), min(max(x0, x1) + r, W - 1)
        by0, by1 = max(min(y0, y1) - r, 0), min(max(y0, y1) + r, H - 1)
        if bx1 < bx0 or by1 < by0:
            continue
        dx, dy = x1 - x0, y1 - y0
        len2 = dx * dx + dy * dy
        if len2 == 0 and m == "zero_length_skipped":
            continue
        box = (xx >= bx0) & (xx <= bx1) & (yy >= by0) & (yy <= by1)
        px, py = xx - x0, yy - y0
        dot = px * dx + py * dy
        first = (len2 == 0) | (dot <= 0)
        second = ~first & (dot >= len2)
        num = np.where(first, px * px + py * py, np.where(second, (xx - x1) ** 2 + (yy - y1) ** 2, (px * dy - py * dx) ** 2))
        den = np.where(first | second, 1, len2)
        masks[lane][box & (16 * num <= width2 * width2 * den)] = 255
    return masks


def pair_counts(masks, G, P, mutant=None):
    """lane_iou_kernel: masks uint8 [G + P, HW] (ground truths first; any non-zero byte is set) -> inter int64 [G, P] = |g & p|,
    area int64 [G + P] = |mask|.  The kernel packs the lanes of a pixel into two 32-bit words: lane 31 is bit 31."""
    m = _mut("pair_counts", mutant)
    b = np.asarray(masks).reshape(G + P, -1) != 0
    g, p = b[:G].copy(), b[G:].copy()
    if m == "bit31_lost":
        g[31:], p[31:] = False, False
    inter = g.astype(np.int64) @ p.astype(np.int64).T
    return inter, np.concatenate([g.sum(1), p.sum(1)]).astype(np.int64)
