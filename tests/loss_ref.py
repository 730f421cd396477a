"""TEST REFERENCE (not part of the product package): the loss kernels of csrc/hn_loss.hip restated in plain numpy -- float64 for values and
gradients, integers for every selection -- plus the seeded inputs that tests/test_loss_ref_cpu.py (which pins these functions to torch
double and to np.sort, and checks the inputs' margins) and tests/test_loss_exact_gpu.py (which holds the kernels to them) share.

Selections are stated on integers: the seg loss's top-k works on the uint32 bit pattern of its non-negative fp32 losses, the lane OHEM on
the order-preserving uint32 key of its fp32 log-probabilities.  A test that reads the kernel's own fp32 losses back can therefore demand
the kernel's threshold, rank remainder and tie count bit for bit."""
import numpy as np

F64 = np.float64


# ------------------------------------------------------------------------------------------------------------------------------------
# top-k selection
# ------------------------------------------------------------------------------------------------------------------------------------
def topk_select(keys, k):
    """keys: 1-D array of sortable values (uint32 bit patterns, or float64 losses), 1 <= k <= len(keys) ->
    (thr, remaining, ties): thr = the k-th largest key, remaining = k - #(keys > thr), ties = #(keys == thr); 1 <= remaining <= ties."""
    keys = np.asarray(keys).reshape(-1)
    n = keys.size
    assert 1 <= k <= n, (k, n)
    thr = np.partition(keys, n - k)[n - k]
    above = int((keys > thr).sum())
    return thr, int(k) - above, int((keys == thr).sum())


def topk_weights(keys, k):
    """The kernel's tie contract as a weight per element: 1 above thr, remaining / ties AT thr, 0 below.  This is not torch.sort's
    contract: a sort keeps an arbitrary `remaining` of the tied elements with weight 1 and drops the others.  The mean is the same
    either way (the tied elements are equal), the gradient is not: here every tied element receives the same share.
    keys [N, HW] -> float64 weights [N, HW], each row summing to k."""
    keys = np.asarray(keys)
    w = np.zeros(keys.shape, F64)
    for n in range(keys.shape[0]):
        thr, remaining, ties = topk_select(keys[n], k)
        w[n] = np.where(keys[n] > thr, 1.0, np.where(keys[n] == thr, remaining / ties, 0.0))
    return w


def f32_bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------------------------------------------
# segmentation losses
# ------------------------------------------------------------------------------------------------------------------------------------
def _softmax(logits):
    z = logits - logits.max(axis=-1, keepdims=True)
    e = np.exp(z)
    s = e.sum(axis=-1, keepdims=True)
    return e / s, z - np.log(s)


def seg_valid(target, C, ignore_index=255):
    """class ids outside [0, C) count as ignored, as the kernel documents (F.cross_entropy raises on them)"""
    t = np.asarray(target).astype(np.int64)
    return (t != ignore_index) & (t >= 0) & (t < C)


def seg_ce(logits, target, cw, ignore_index=255):
    """weighted cross entropy per pixel.  logits [..., C] float64, target [...] class ids, cw [C] ->
    (loss [...], dloss [..., C]): loss = cw[y] (logsumexp(l) - l[y]) and 0 for ignored pixels; dloss = its gradient w.r.t. the logits"""
    logits = np.asarray(logits, F64)
    cw = np.asarray(cw, F64)
    C = logits.shape[-1]
    valid = seg_valid(target, C, ignore_index)
    y = np.where(valid, np.asarray(target).astype(np.int64), 0)
    sm, lsm = _softmax(logits)
    wy = np.where(valid, cw[y], 0.0)
    loss = -wy * np.take_along_axis(lsm, y[..., None], -1)[..., 0]
    onehot = np.arange(C) == y[..., None]
    return loss, wy[..., None] * (sm - onehot)


def seg_ce_mean(logits, target, cw, use_topk, k, ignore_index=255, keys=None):
    """logits [N, HW, C], target [N, HW] -> (scalar, d scalar / d logits).  use_topk: the mean of the k largest losses of every image
    under topk_weights' tie contract (keys: what to select on, default the float64 losses), else the mean over all N * HW pixels."""
    loss, dloss = seg_ce(logits, target, cw, ignore_index)
    if use_topk:
        w = topk_weights(loss if keys is None else keys, k)
        denom = loss.shape[0] * k
    else:
        w = np.ones_like(loss)
        denom = loss.size
    return float((w * loss).sum() / denom), dloss * (w / denom)[..., None]


def seg_focal(logits, target, cw, gamma, alpha):
    """focal seg loss: p = softmax + 1e-8, t = onehot + 1e-8, loss = mean over pixels of sum_c t_c (-alpha (1 - p_c)^gamma log p_c cw_c)
    (no ignore_index on this path).  1 - p is clamped at 0: in float64 a saturated pixel has p = 1 + 1e-8 - O(e^-60) > 1, and a
    negative base has no real power for a fractional gamma (torch returns NaN); in fp32, the arithmetic this loss was defined in,
    1 + 1e-8 is 1 and the base is exactly 0.  For gamma 1 and 2 the clamp moves the loss by at most 1e-16.
    logits [M, C], target [M] -> (scalar, gradient [M, C])"""
    logits = np.asarray(logits, F64)
    cw = np.asarray(cw, F64)
    M, C = logits.shape
    sm, _ = _softmax(logits)
    p = sm + 1e-8
    q = np.maximum(1.0 - p, 0.0)
    t = (np.arange(C) == np.asarray(target).astype(np.int64)[:, None]) + 1e-8
    loss = (t * (-alpha * q ** gamma * np.log(p) * cw)).sum(-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        qg1 = np.where(q > 0, q ** (gamma - 1.0), 1.0 if gamma == 1.0 else 0.0)
    g = t * cw * alpha * (gamma * qg1 * np.log(p) - q ** gamma / p)          # d loss_pix / d p_c
    dot = (g * sm).sum(-1, keepdims=True)
    return float(loss.mean()), sm * (g - dot) / M


def s2d_channels(d, N, H, W, C, ldz):
    """dlogits [N*H*W, C] -> the space-to-depth operand [N, H/2, W/2, ldz]: channel (py*2+px)*C + c of low-res pixel (y, x) =
    dlogits(2y+py, 2x+px, c), zeros in [4C, ldz)"""
    d = np.asarray(d).reshape(N, H // 2, 2, W // 2, 2, C).transpose(0, 1, 3, 2, 4, 5).reshape(N, H // 2, W // 2, 4 * C)
    out = np.zeros((N, H // 2, W // 2, ldz), d.dtype)
    out[..., :4 * C] = d
    return out


def bf16_line(x):
    """float values -> their bf16 roundings as integers on a line: equal values (+0 and -0 too) map to equal integers and neighbouring
    bf16 values to neighbouring integers"""
    import torch
    v = torch.from_numpy(np.asarray(x, np.float64)).to(torch.bfloat16).view(torch.int16).numpy().astype(np.int64)
    return np.where(v < 0, -(v & 0x7FFF), v)


def focal_case(C, m=300, saturated=True):
    """inputs of the focal tests: logits randn * 3 [m, C], targets, class weights; saturated: the first six pixels have one logit at
    +30 and the others at -30, the first two with the hot class as target, the next two (at least) with another"""
    g = np.random.default_rng(C)
    logits = (g.standard_normal((m, C)) * 3).astype(np.float32)
    target = g.integers(0, C, m).astype(np.int64)
    if saturated:
        logits[:6] = -30.0
        logits[np.arange(6), np.arange(6) % C] = 30.0
        target[:6] = np.array([0, 1, 1, 0, 1, 0])
    cw = (g.random(C) * 2 + 0.2).astype(np.float32)
    return logits, target, cw


def seg_case(seed, C, n, h, w):
    """the random inputs of the seg CE tests: logits randn * 2 (fp32 values), targets with a block of 255, a few ids equal to C and -1,
    class weights with one 0.0 -> (logits fp32 [n, h*w, C], target int64 [n, h*w], cw fp32 [C])"""
    g = np.random.default_rng(1000 * seed + 16 * (n * h * w) + C)
    hw = h * w
    logits = (g.standard_normal((n, hw, C)) * 2).astype(np.float32)
    target = g.integers(0, C, (n, hw)).astype(np.int64)
    target[0, :max(hw // 10, 2)] = 255
    target[n - 1, hw // 2:hw // 2 + 3] = C
    target[0, hw - 3:] = -1
    cw = np.round(g.uniform(0.1, 5.0, C), 2).astype(np.float32)
    cw[C // 2] = 0.0
    return logits, target, cw


def choose_k(loss):
    """loss float64 [N, HW] -> (k, gap): among the ranks k in [0.25 HW, 0.35 HW] the one whose relative gap between the k-th and the
    (k+1)-th largest loss, minimised over the images, is largest"""
    hw = loss.shape[1]
    s = -np.sort(-loss, axis=1)
    lo, hi = int(np.ceil(0.25 * hw)), int(np.floor(0.35 * hw))
    ks = np.arange(max(lo, 1), min(hi, hw - 1) + 1)
    gaps = ((s[:, ks - 1] - s[:, ks]) / s[:, ks - 1]).min(axis=0)
    i = int(np.argmax(gaps))
    return int(ks[i]), float(gaps[i])


# ------------------------------------------------------------------------------------------------------------------------------------
# lane losses
# ------------------------------------------------------------------------------------------------------------------------------------
def f2ord(bits):
    """order-preserving uint32 key of fp32 bit patterns (negative values complemented, the others get the top bit)"""
    bits = np.asarray(bits, np.uint32)
    return np.where(bits & np.uint32(0x80000000), ~bits, bits | np.uint32(0x80000000)).astype(np.uint32)


def ord2f(key):
    key = np.uint32(key)
    u = (key & np.uint32(0x7FFFFFFF)) if key & np.uint32(0x80000000) else ~key
    return np.array([u], np.uint32).view(np.float32)[0]


def lane_counts(target, neg_ratio=15.0):
    """one-hot targets [M, 2] -> (pmask bool [M], npos, nneg, k): k = clamp(neg_ratio * #pos, 1, #neg) as the 1-based rank of the OHEM
    threshold among the negatives' background log-probs"""
    pmask = np.asarray(target)[:, 1] > 0
    npos, nneg = int(pmask.sum()), int((~pmask).sum())
    return pmask, npos, nneg, int(max(min(npos * neg_ratio, nneg), 1))


def lane_select(bg_f32, pmask, k):
    """the k-th smallest of the negatives' fp32 background log-probs, selected on their integer keys; +inf without negatives"""
    keys = f2ord(f32_bits(bg_f32)[~pmask])
    if keys.size == 0:
        return np.float32(np.inf)
    return ord2f(np.partition(keys, k - 1)[k - 1])


def lane_cls(logits, target, neg_ratio=15.0, alpha=10.0, gpos=1.0, gneg=1.0):
    """OHEM lane classification loss in float64.  logits [M, 2], one-hot target [M, 2] ->
    dict(pos, neg, thr, posn, npos, nneg, pmask, lsm, dlogits): pos = -alpha sum_pos log p_fg / max(#pos, 1),
    neg = -alpha sum_{neg, log p_bg <= thr} log p_bg / max(#pos, 1); dlogits = gpos d pos + gneg d neg (thr is a constant)"""
    z = np.asarray(logits, F64)
    pmask, npos, nneg, k = lane_counts(target, neg_ratio)
    sm, lsm = _softmax(z)
    bg, fg = lsm[:, 0], lsm[:, 1]
    thr = np.partition(bg[~pmask], k - 1)[k - 1] if nneg else np.inf
    hard = ~pmask & (bg <= thr)
    posn = max(npos, 1)
    d = np.zeros_like(z)
    cp, cn = -alpha / posn * gpos, -alpha / posn * gneg
    d[pmask] = cp * (np.array([0.0, 1.0]) - sm[pmask])
    d[hard] = cn * (np.array([1.0, 0.0]) - sm[hard])
    return dict(pos=-alpha * fg[pmask].sum() / posn, neg=-alpha * bg[hard].sum() / posn, thr=thr, posn=posn, npos=npos, nneg=nneg,
                pmask=pmask, lsm=lsm, dlogits=d, k=k)


def lane_loc(pred, target, pmask, posn, wcol, alpha=10.0, gout=1.0):
    """masked Huber location loss in float64: per positive row sum_c huber(p - t) w_c [t != 0] / max(#[t != 0], 1), w = alpha at columns
    wcol and wcol + 1, summed over the rows and divided by posn.  -> (loss, dpred, rownorm)"""
    p, t = np.asarray(pred, F64), np.asarray(target, F64)
    L = p.shape[1]
    wgt = np.ones(L)
    wgt[wcol] = wgt[wcol + 1] = alpha
    mask = (t != 0) * np.asarray(pmask, bool)[:, None] * wgt
    nrm = np.maximum((t != 0).sum(1), 1).astype(F64)
    d = p - t
    ad = np.abs(d)
    hub = np.where(ad < 1, d * d / 2, ad - 0.5)
    loss = ((hub * mask).sum(1) / nrm).sum() / posn
    dh = np.where(ad < 1, d, np.sign(d))
    return float(loss), dh * mask / nrm[:, None] / posn * gout, nrm


def lane_loc_case(L_, M=37, wcol=1):
    """inputs of the lane location tests (fp32 values): targets on a 1/8 grid with ~30 % zeros (invalid points), rows 3 and M - 1 without
    a single valid point, and positives whose |pred - target| is exactly 1, one ulp below and one ulp above (rows 0 and 5)
    -> (pred [M, L], target [M, L], pmask bool [M], posn)"""
    g = np.random.default_rng(L_ * 100 + wcol)
    t = (g.integers(-40, 41, (M, L_)) / 8.0).astype(np.float32) * (g.random((M, L_)) < 0.7)
    t[3] = 0.0                                                               # rows without a single valid point
    t[M - 1] = 0.0
    p = (t + g.standard_normal((M, L_)) * 1.5).astype(np.float32)
    pmask = g.random(M) < 0.5
    pmask[[0, 3, 5]] = True
    t[0, :3], t[5, :3] = -0.5, 0.5                                            # pred = -+0.5 +- edge is exact in fp32, so pred - target is the edge
    p[0, :3] = t[0, :3] + LOC_EDGES[:min(3, L_)]
    p[5, :3] = t[5, :3] - LOC_EDGES[:min(3, L_)]
    return p.astype(np.float32), t.astype(np.float32), pmask, float(max(pmask.sum(), 1))


LOC_EDGES = np.array([1.0, 1.0 - 2.0 ** -24, 1.0 + 2.0 ** -23], np.float32)  # |pred - target| at the Huber knee, one ulp below and above


# ------------------------------------------------------------------------------------------------------------------------------------
# smooth-L1 detection loss
# ------------------------------------------------------------------------------------------------------------------------------------
def det_iou(anchors, ann):
    """anchors [A, 4] (y1, x1, y2, x2), ann [Mx, 5] (x1, y1, x2, y2, class; class -1 = padding) of ONE image, float64 ->
    IoU [A, Mx] with -1 in the padding columns (the formula of tests/det_iou_ref.assign)"""
    a, b = np.asarray(anchors, F64), np.asarray(ann, F64)
    iw = np.maximum(np.minimum(a[:, None, 3], b[None, :, 2]) - np.maximum(a[:, None, 1], b[None, :, 0]), 0)
    ih = np.maximum(np.minimum(a[:, None, 2], b[None, :, 3]) - np.maximum(a[:, None, 0], b[None, :, 1]), 0)
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    ua = ((a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1]))[:, None] + area[None, :] - iw * ih
    iou = iw * ih / np.maximum(ua, 1e-8)
    return np.where(b[None, :, 4] != -1, iou, -1.0)


def det_margins(anchors, ann):
    """anchors [A, 4], ann [N, Mx, 5] -> (distance of any anchor's best IoU from 0.4 / 0.5, smallest best - second-best gap among the
    anchors whose best IoU is positive and that see two valid boxes): the assignment is the same in fp32 and float64 while both are
    well above the fp32 error of an IoU"""
    thr_m, gap_m = np.inf, np.inf
    for n in range(ann.shape[0]):
        iou = det_iou(anchors, ann[n])
        if not (np.asarray(ann[n])[:, 4] != -1).any():
            continue
        s = -np.sort(-iou, axis=1)
        best = s[:, 0]
        thr_m = min(thr_m, float(np.abs(best - 0.4).min()), float(np.abs(best - 0.5).min()))
        if s.shape[1] > 1:
            two = (best > 0) & (s[:, 1] >= 0)
            if two.any():
                gap_m = min(gap_m, float((best - s[:, 1])[two].min()))
    return thr_m, gap_m


def det_smooth_l1(cls, reg, anchors, ann, gcls=1.0, greg=1.0):
    """The detection loss with the smooth-L1 (beta 1/9) regression term, float64.  cls [N, A, K] probabilities, reg [N, A, 4],
    anchors [A, 4], ann [N, Mx, 5].  Anchor assignment is tests/det_iou_ref.assign's (IoU >= 0.5 positive, first maximum wins, an image
    without boxes all background); background = best IoU < 0.4, the rest is ignored.  ->
    dict(cls, reg, npos [N], assign [N, A] (index | -1 | -2), dcls, dreg): gradients of gcls * cls + greg * reg"""
    import torch
    from tests import det_iou_ref as R
    cls, reg, anc, ann = (np.asarray(v, F64) for v in (cls, reg, anchors, ann))
    N, A, K = cls.shape
    c = np.clip(cls, 1e-4, 1.0 - 1e-4)
    inside = (cls > 1e-4) & (cls < 1.0 - 1e-4)                                # the clamp has zero slope outside its range
    aw, ah = anc[:, 3] - anc[:, 1], anc[:, 2] - anc[:, 0]
    acx, acy = anc[:, 1] + 0.5 * aw, anc[:, 0] + 0.5 * ah
    out_c, out_r, npos, assign = 0.0, 0.0, [], np.full((N, A), -1, np.int64)
    dcls, dreg = np.zeros_like(cls), np.zeros_like(reg)
    for n in range(N):
        pos, arg = R.assign(torch.from_numpy(anc), torch.from_numpy(ann[n]))
        pos, arg = pos.numpy(), arg.numpy()
        has = bool((ann[n][:, 4] != -1).any())
        best = det_iou(anc, ann[n]).max(axis=1)
        neg = (best < 0.4) | (not has)
        assign[n] = np.where(pos, arg, np.where(neg, -1, -2))
        p = int(pos.sum())
        npos.append(p)
        onehot = pos[:, None] & (ann[n][arg, 4].astype(np.int64)[:, None] == np.arange(K)[None, :])
        counted = (pos | neg)[:, None]
        cn = c[n]
        focal = np.where(onehot, 0.25 * (1 - cn) ** 2 * -np.log(cn), 0.75 * cn ** 2 * -np.log(1 - cn))
        out_c += np.where(counted, focal, 0.0).sum() / max(p, 1) / N
        gf = np.where(onehot, 0.25 * (2 * (1 - cn) * np.log(cn) - (1 - cn) ** 2 / cn), 0.75 * (-2 * cn * np.log(1 - cn) + cn ** 2 / (1 - cn)))
        dcls[n] = np.where(counted & inside[n], gf, 0.0) * gcls / (N * max(p, 1))
        if p:
            b = ann[n][arg]
            gw, gh = b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]
            gcx, gcy = b[:, 0] + 0.5 * gw, b[:, 1] + 0.5 * gh
            gw, gh = np.maximum(gw, 1.0), np.maximum(gh, 1.0)
            t = np.stack([(gcy - acy) / ah, (gcx - acx) / aw, np.log(gh / ah), np.log(gw / aw)], 1)
            d = t - reg[n]
            ad = np.abs(d)
            rl = np.where(ad <= 1.0 / 9.0, 0.5 * 9.0 * ad ** 2, ad - 0.5 / 9.0)
            out_r += (rl * pos[:, None]).sum() / (4.0 * p) / N
            dreg[n] = np.where(ad <= 1.0 / 9.0, -9.0 * d, -np.sign(d)) * pos[:, None] * greg / (N * 4.0 * p)
    return dict(cls=float(out_c), reg=float(out_r), npos=npos, assign=assign, dcls=dcls, dreg=dreg)


def grid_anchors(levels=((32, 128.0), (16, 64.0), (8, 32.0)), hw=(128, 256), ratios=((1.0, 1.0), (0.7, 1.4), (1.4, 0.7))):
    """(y1, x1, y2, x2) anchors of a small multi-scale grid, coarse level first; stride = size / 4, so a box has several positives"""
    out = []
    for stride, size in levels:
        for y in range(stride // 2, hw[0], stride):
            for x in range(stride // 2, hw[1], stride):
                for rh, rw in ratios:
                    out.append([y - size * rh / 2, x - size * rw / 2, y + size * rh / 2, x + size * rw / 2])
    return np.array(out, np.float32)


def det_case(N, A, K, Mx=8):
    """fp32 inputs of the smooth-L1 tests: the first A anchors of grid_anchors(); every image's boxes are perturbed copies of distinct
    anchors (corners moved by up to 6 % of the side, IoU with the source > 0.75), the other annotation rows are -1 padding and, for
    N > 1, image 1 has no box at all; a few probabilities sit exactly at 0 and 1 (the clamp)."""
    g = np.random.default_rng(100000 * N + 100 * A + K)
    anc = grid_anchors()[:A].copy()
    assert anc.shape[0] == A
    ann = np.full((N, Mx, 5), -1.0, np.float32)
    for n in range(N):
        if N > 1 and n == 1:
            continue
        for _ in range(1000):                                             # redrawn until the image keeps the margins of det_margins
            ann[n] = -1.0
            nb = min(A, int(g.integers(1, 6)))
            for j, i in enumerate(g.choice(A, nb, replace=False)):
                y1, x1, y2, x2 = anc[i]
                h, w = y2 - y1, x2 - x1
                d = (g.random(4) - 0.5) * 0.12
                ann[n, j] = [x1 + d[0] * w, y1 + d[1] * h, x2 + d[2] * w, y2 + d[3] * h, float(g.integers(0, K))]
            if min(det_margins(anc, ann[n:n + 1])) > 3e-4:
                break
        else:
            raise AssertionError("no draw keeps the margins")
    cls = (g.random((N, A, K)) * 0.98 + 0.01).astype(np.float32)
    cls.reshape(-1)[::37] = 0.0
    cls.reshape(-1)[5::41] = 1.0
    reg = (g.standard_normal((N, A, 4)) * 0.2).astype(np.float32)
    return cls, reg, anc, ann


# ------------------------------------------------------------------------------------------------------------------------------------
# weighted loss sum
# ------------------------------------------------------------------------------------------------------------------------------------
def weighted_sum(x, w, gw, grp, gout=1.0):
    """total = sum_g (sum_{i in g} x_i w_i) gw_g, left to right, every product and sum rounded to fp32 on its own; gradients
    (gout gw_g) w_i likewise.  x, w [n], gw indexed by group id, grp [n] ascending -> (np.float32 total, np.float32 grads [n])"""
    f = np.float32
    x, w, gw = (np.asarray(v, f) for v in (x, w, gw))
    tot, i, n = f(0), 0, len(x)
    while i < n:
        g = grp[i]
        s = f(x[i] * w[i])
        i += 1
        while i < n and grp[i] == g:
            s = f(s + f(x[i] * w[i]))
            i += 1
        tot = f(tot + f(s * gw[g]))
    grads = np.array([f(f(f(gout) * gw[grp[i]]) * w[i]) for i in range(n)], f)
    return tot, grads


def weighted_sum_other_orders(x, w, gw, grp):
    """the same total associated differently: (right to left in fp32, the float64 total rounded once)"""
    f = np.float32
    x, w, gw = (np.asarray(v, f) for v in (x, w, gw))
    rev = f(0)
    for g in sorted(set(grp), reverse=True):
        s = f(0)
        for i in reversed(np.nonzero(np.asarray(grp) == g)[0]):
            s = f(s + f(x[i] * w[i]))
        rev = f(rev + f(s * gw[g]))
    exact = sum(float(gw[g]) * float((x.astype(F64) * w.astype(F64))[np.asarray(grp) == g].sum()) for g in set(grp))
    return rev, f(exact)


def weighted_sum_case(n, groups):
    """fp32 terms and weights drawn until (for n > 1) another association order changes the total's last bits"""
    g = np.random.default_rng(10 * n + groups)
    grp = np.sort(np.arange(n) % groups).astype(np.int32)
    while True:
        x = (g.random(n) * 3 + 0.1).astype(np.float32)
        w = (g.random(n) * 2 + 0.3).astype(np.float32)
        gw = (g.random(groups) * 2 + 0.5).astype(np.float32)
        tot = weighted_sum(x, w, gw, grp)[0]
        if n == 1 or all(v != tot for v in weighted_sum_other_orders(x, w, gw, grp)):
            return x, w, gw, grp


# ------------------------------------------------------------------------------------------------------------------------------------
# injected bit patterns: a seg pixel with logits (0, -b, ..., -b), target 1 and cw[1] = 1 has the loss b exactly for any fp32 b >= 32
# (exp(-b) vanishes against 1 and log 1 = 0); with target 0 it has the loss 0.  A lane row (-b, 0) has the background log-prob -b.
# ------------------------------------------------------------------------------------------------------------------------------------
SEG_PATTERNS = ("equal", "low10", "mid11", "top", "ties", "sparse", "ignored")


def seg_pattern(name, HW):
    """-> (b fp32 [HW]: the loss to inject, 0 = a valid pixel with loss 0; ignored bool [HW]; ks: the ranks to select) or None when the
    pattern does not fit into HW pixels.  Values are spread over the image by a fixed permutation, so with two blocks per image both
    blocks hold part of every group.
      equal   all values equal: ties = HW, remaining = k
      low10   32 + j 2^-18, j < 1024 (bits 9..0 only): k puts the threshold at j in {0, 15, 16, 1023}, level-2 chunk edges and bin 0
      mid11   32 + j 2^-8, j < 2048 (bits 20..10 only): threshold at j in {0, 31, 32, 2016, 2047}, level-1 chunk edges and bin 0
      top     {1, 1.25, 1.5, 1.75} 2^e, e = 5..20, one value per level-0 bin with zero low bits: k in {1, HW} and level-0 chunk edges
      ties    a values above a group of T copies, the rest below: k in {a + 1, a + T/2, a + T}
      sparse  60 % ignored, 20 % valid with loss 0, the rest injected: k just above the number of non-zero losses
      ignored every pixel ignored"""
    g = np.random.default_rng(HW * 31 + SEG_PATTERNS.index(name))
    b = np.zeros(HW, np.float32)
    ign = np.zeros(HW, bool)
    perm = g.permutation(HW)

    def place(vals):
        vals = np.asarray(vals, np.float32)
        if vals.size > HW:
            return False
        b[perm[:vals.size]] = vals
        return True
    if name == "equal":
        b[:] = 40.0
        return b, ign, sorted({1, (HW + 1) // 2, HW})
    if name == "low10":
        return (b, ign, [1024 - j for j in (0, 15, 16, 1023)]) if place(32.0 + np.arange(1024) * 2.0 ** -18) else None
    if name == "mid11":
        return (b, ign, [2048 - j for j in (0, 31, 32, 2016, 2047)]) if place(32.0 + np.arange(2048) * 2.0 ** -8) else None
    if name == "top":
        vals = [m * 2.0 ** e for e in range(5, 21) for m in (1.0, 1.25, 1.5, 1.75)]
        return (b, ign, sorted({1, HW, 64, 64 - 15, 64 - 16, 64 - 47, 64 - 48})) if place(vals) else None
    if name == "ties":
        if HW < 4:
            return None
        a, T = HW // 8, HW // 4
        below = HW - a - T - HW // 3                                     # the last third stays at loss 0
        place(np.concatenate([64.0 + np.arange(a) * 2.0 ** -10, np.full(T, 36.0), 32.0 + np.arange(below) * 2.0 ** -12]))
        return b, ign, sorted({a + 1, a + max(T // 2, 1), a + T})
    if name == "sparse":
        if HW < 200:
            return None
        n_ign, n_zero = (HW * 6) // 10, (HW * 2) // 10
        nnz = HW - n_ign - n_zero
        ign[perm[nnz:nnz + n_ign]] = True
        place(32.0 + g.integers(0, 1 << 20, nnz) * 2.0 ** -16)
        return b, ign, sorted({nnz + 1, min(nnz + 7, HW)})
    if name == "ignored":
        ign[:] = True
        return b, ign, sorted({1, (HW + 1) // 2, HW})
    raise ValueError(name)


def seg_inject(images, C=5):
    """images: list of (b, ignored) -> (logits fp32 [N, HW, C], target int64 [N, HW], cw fp32 [C])"""
    N, HW = len(images), images[0][0].size
    logits = np.zeros((N, HW, C), np.float32)
    target = np.zeros((N, HW), np.int64)
    for n, (b, ign) in enumerate(images):
        logits[n, :, 1:] = -np.where(b > 0, b, 40.0)[:, None]
        target[n] = np.where(ign, 255, np.where(b > 0, 1, 0))
    cw = np.array([0.5, 1.0, 2.0, 0.25, 3.0, 0.7, 1.5, 0.9, 1.1, 0.3, 2.5, 0.6, 1.7, 0.8, 1.3, 0.4][:C], np.float32)
    return logits, target, cw


LANE_PATTERNS = ("lowbyte", "topbyte", "ties", "every_negative", "no_positive", "no_negative")


def lane_pattern(name, M):
    """-> list of (logits fp32 [M, 2], one-hot target fp32 [M, 2], neg_ratio, injected: bool [M] rows of the form (-b, 0)).  The
    injected negatives have the smallest background log-probs (all other negatives have random logits, log p_bg > -32), and with
    neg_ratio = 1 the rank of the threshold is the number of positives.
      lowbyte        b = 32 + j 2^-18, j < 256 (keys differ in the lowest byte): k in {1, 64, 65, 128}, the wave edges of the bin scan
      topbyte        b = 2^e, e = 5, 7, ..., 99 (one key per top byte): k in {1, 2, 47, 48}
      ties           20 distinct values above 100 copies of one value: k in {21, 70, 120}, the last with the group exactly used up
      every_negative neg_ratio 15 and 15 #pos >= #neg: k = #neg, the threshold is the largest negative
      no_positive    k clamps to 1
      no_negative    thr = +inf, neg = 0"""
    g = np.random.default_rng(M * 7 + LANE_PATTERNS.index(name))
    out = []

    def case(inj_b, npos, ratio):
        z = g.standard_normal((M, 2)).astype(np.float32)
        perm = g.permutation(M)
        inj = np.zeros(M, bool)
        ni = len(inj_b)
        assert ni + npos <= M
        z[perm[:ni], 0] = -np.asarray(inj_b, np.float32)
        z[perm[:ni], 1] = 0.0
        inj[perm[:ni]] = True
        fg = np.zeros(M, bool)
        fg[perm[ni:ni + npos]] = True
        t = np.stack([~fg, fg], 1).astype(np.float32)
        out.append((z, t, ratio, inj))
    if name == "lowbyte":
        for k in (1, 64, 65, 128):
            case(32.0 + np.arange(256) * 2.0 ** -18, k, 1.0)
    elif name == "topbyte":
        for k in (1, 2, 47, 48):
            case(2.0 ** np.arange(5, 100, 2), k, 1.0)
    elif name == "ties":
        for k in (21, 70, 120):
            case(np.concatenate([64.0 + np.arange(20), np.full(100, 36.0)]), k, 1.0)
    elif name == "every_negative":
        case(32.0 + np.arange(16), M // 12, 15.0)
    elif name == "no_positive":
        case(32.0 + np.arange(16) * 2.0 ** -18, 0, 15.0)
    elif name == "no_negative":
        case([], M, 15.0)
    else:
        raise ValueError(name)
    return out
