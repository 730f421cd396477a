"""fp64 torch restatement of the Lovasz-softmax seg loss contract (segment.use_lovasz), written from the formulas: differentiable, with the
stable descending sort that defines the kernels' order inside ties.  Runs on CPU and GPU.

    p = softmax(logits) over C; pixels in (n, h, w) order, label == ignore_index dropped, other labels outside [0, C) background;
    per present class c: e = |fg - p_c| sorted descending (ties: pixel index ascending); F_j / B_j running fg / bg counts, G = fg count;
    J_j = 1 - (G - F_j) / (G + B_j); loss_c = sum_j e_(j) (J_j - J_{j-1}), J_{-1} = 0, the J differences held constant;
    loss = mean over present classes (0 with a zero gradient when none is present).

Below it, the exact restatement in numpy (float64 and integers) that tests/test_lovasz_exact_gpu.py holds hn_lovasz.hip's workspace to: the
workspace layout, the sort keys, the properties that define a correct stable sort, the closed-form weights and the per-pixel gradient."""
import numpy as np
import torch

TILE = 8192                    # LV_TILE: pixels per sorted tile
BINS = 1024                    # LV_BINS: digit bins per radix pass
IGNORED_KEY = 0x3FFFFFFF       # LV_IGNORED: the key of an ignored pixel (sorts last)
ONE_KEY = 0x3F800000           # bits of 1.0f, the largest key of a valid pixel
MAXC = 16
WS_ARRAYS = ("keysA", "valsA", "keysB", "valsB", "hist", "totals", "counts", "blkfg", "part")


def lovasz_softmax_ref(logits_nchw, target, ignore_index=255):
    x = logits_nchw.to(torch.float64)
    c = x.shape[1]
    p = torch.softmax(x, 1).permute(0, 2, 3, 1).reshape(-1, c)
    lab = target.reshape(-1).to(torch.int64)
    keep = lab != ignore_index
    p, lab = p[keep], lab[keep]
    losses = []
    for k in range(c):
        fg = (lab == k).to(torch.float64)
        g = fg.sum()
        if g == 0:
            continue
        e = (fg - p[:, k]).abs()
        es, perm = torch.sort(e, descending=True, stable=True)
        fs = fg[perm]
        jac = 1.0 - (g - fs.cumsum(0)) / (g + (1.0 - fs).cumsum(0))
        wgt = torch.cat([jac[:1], jac[1:] - jac[:-1]])
        losses.append((es * wgt.detach()).sum())
    if not losses:
        return (x * 0.0).sum()
    return torch.stack(losses).mean()


# ---- exact restatement of hn_lovasz.hip's intermediate results ----------------------------------------------------------------------------
def _align(x):
    return (x + 255) & ~255


def ws_layout(N, HW, C):
    """byte offsets of the workspace arrays (the layout comment above `struct LvWs`): keysA | valsA | keysB | valsB, u32 [C][P] each |
    hist u32 [C][1024][nblk] | totals u32 [C][1024] | counts u32 [32] (256 bytes) | blkfg u32 [C][nblk] | part fp32 [C][nblk], every array
    aligned to 256 bytes, nblk = ceil(P / 8192).  After the forward the sorted keys / payloads are in keysB / valsB (three passes:
    A -> B -> A -> B) and keysA holds g, fp32 [P][C].  -> {name: offset, "total": bytes, "nblk": tiles, "P": pixels}; a refused shape
    (N <= 0, HW <= 0, C outside [2, 16]) has total 0, as hn_seg_lovasz_ws_bytes answers."""
    if N <= 0 or HW <= 0 or C < 2 or C > MAXC:
        return dict(total=0, nblk=0, P=0)
    P = N * HW
    nblk = -(-P // TILE)
    arr = _align(C * P * 4)
    sizes = (arr, arr, arr, arr, _align(C * BINS * nblk * 4), _align(C * BINS * 4), 256, _align(C * nblk * 4), _align(C * nblk * 4))
    lay, off = dict(nblk=nblk, P=P), 0
    for name, sz in zip(WS_ARRAYS, sizes):
        lay[name] = off
        off += sz
    lay["total"] = off
    return lay


def _rowsum(a):
    """sum over the (short) last axis of [P, C], column by column: much faster than a reduction along an axis of 2..16 elements"""
    s = a[:, 0].copy()
    for k in range(1, a.shape[1]):
        s += a[:, k]
    return s


def _exp64(logits):
    x = np.asarray(logits, np.float64)
    mx = x[:, 0].copy()
    for k in range(1, x.shape[1]):
        np.maximum(mx, x[:, k], out=mx)
    return np.exp(x - mx[:, None])


def softmax64(logits):
    """float64 softmax over the last axis of logits [P, C]"""
    e = _exp64(logits)
    return e / _rowsum(e)[:, None]


def key_d(logits, labels, c):
    """float64 d = 1 - |fg - p_c| per pixel of logits [P, C], labels int [P]: p_c for a fg pixel (label == c), 1 - p_c otherwise -- the
    latter formed as the other classes' share of the softmax sum, so that a d near 0 keeps its relative precision"""
    e = _exp64(logits)
    oth = np.zeros(e.shape[0])
    for k in range(e.shape[1]):
        if k != c:
            oth += e[:, k]
    return np.where(np.asarray(labels) == c, e[:, c], oth) / (oth + e[:, c])


def check_sorted(keys_sorted, vals_sorted, labels, valid, c, d64):
    """the properties that define class c's correct stable sort, asserted on the sorted keys / payloads u32 [P] (payload = pixel index
    | fg << 31); labels int [P], valid bool [P], d64 = key_d(...) float64 [P].  No order of near-equal floats is predicted: the keys the
    device formed are held to d64 within 4e-6 relative (or 1e-37 absolute: an fp32 underflow), the order to the device's own keys.
      whole array   (key, pixel index) strictly increasing: the keys never decrease, equal keys keep the pixel order (stability)
      j < V         the pixels are exactly the valid ones, each once; bit 31 is label == c; key <= bits(1.0f) and float(key) ~ d64[pixel]
      j >= V        key 0x3FFFFFFF, the pixels are the ignored ones, bit 31 clear"""
    k = np.asarray(keys_sorted).astype(np.int64)
    v = np.asarray(vals_sorted).astype(np.int64)
    valid = np.asarray(valid, bool)
    labels = np.asarray(labels)
    P, V = k.shape[0], int(valid.sum())
    assert v.shape == (P,) and valid.shape == (P,) and labels.shape == (P,), (k.shape, v.shape, valid.shape, labels.shape)
    pix, fgb = v & 0x7FFFFFFF, v >> 31

    def first(bad):
        j = int(np.flatnonzero(bad)[0])
        return f"class {c}: first at sorted position {j} of {P} (V = {V}): key 0x{int(k[j]):08x} payload 0x{int(v[j]):08x}"

    bad = pix >= P
    assert not bad.any(), "payload names a pixel outside the map; " + first(bad)
    bad = np.diff(k[:V]) < 0
    assert not bad.any(), "keys decrease; " + first(bad)
    bad = np.diff((k << 31) | pix) <= 0
    assert not bad.any(), "(key, pixel index) does not increase strictly (a lost stable order or a repeated item); " + first(bad)
    assert np.array_equal(np.sort(pix[:V]), np.flatnonzero(valid)), f"class {c}: the first V = {V} payloads are not the valid pixels, each once"
    assert np.array_equal(np.sort(pix[V:]), np.flatnonzero(~valid)), f"class {c}: the payloads past V = {V} are not the ignored pixels"
    bad = k[:V] > ONE_KEY
    assert not bad.any(), "a valid pixel's key is above 1.0f; " + first(bad)
    bad = np.concatenate([np.zeros(V, bool), k[V:] != IGNORED_KEY])
    assert not bad.any(), "an ignored pixel's key is not 0x3FFFFFFF; " + first(bad)
    bad = fgb != np.concatenate([labels[pix[:V]] == c, np.zeros(P - V, bool)])
    assert not bad.any(), "bit 31 of the payload is not (label == c); " + first(bad)
    kf = np.asarray(keys_sorted)[:V].astype(np.uint32).view(np.float32).astype(np.float64)
    want = np.asarray(d64, np.float64)[pix[:V]]
    err = np.abs(kf - want)
    bad = ~((err <= 4e-6 * np.abs(want)) | (err <= 1e-37))
    if bad.any():
        j = int(np.flatnonzero(bad)[0])
        raise AssertionError(f"key is not d = 1 - |fg - p_c|; {first(bad)}: float(key) {kf[j]!r}, float64 d {want[j]!r}")


def weights(fg_sorted, G):
    """fg_sorted bool [V] along the sorted order, G = fg count -> exact F, B int64 [V] (fg / bg pixels in FRONT of position j, so
    F + B = j) and the float64 weights J_j - J_{j-1}, J_j = 1 - (G - F_j - fg_j) / (G + B_j + 1 - fg_j): 1 / (G + B) at a fg position,
    (G - F) / ((G + B)(G + B + 1)) at a bg one"""
    fg = np.asarray(fg_sorted, bool)
    F = np.cumsum(fg, dtype=np.int64) - fg
    B = np.arange(fg.shape[0], dtype=np.int64) - F
    gb = (G + B).astype(np.float64)
    w = np.where(fg, 1.0 / gb, (G - F).astype(np.float64) / (gb * (gb + 1.0)))
    return F, B, w


def _masked_g(g, present):
    return np.where(np.asarray(present, bool)[None, :], np.asarray(g, np.float64), 0.0)


def pixel_grad(logits, g, present, scale):
    """float64 dlogits [P, C] = scale * p_c * (g_c - sum_k p_k g_k), the sum over the present classes and g_c taken as 0 for an absent
    one (g [P, C] is the gradient with respect to the probabilities; its entries for absent classes are never read)"""
    p = softmax64(logits)
    gm = _masked_g(g, present)
    return scale * p * (gm - _rowsum(p * gm)[:, None])


def pixel_grad_mag(logits, g, present, scale):
    """|scale| * p_c * (|g_c| + sum_k p_k |g_k|): the magnitude of what pixel_grad's components are formed from (the error bound of an
    fp32 evaluation is a multiple of it)"""
    p = softmax64(logits)
    gm = np.abs(_masked_g(g, present))
    return abs(scale) * p * (gm + _rowsum(p * gm)[:, None])
