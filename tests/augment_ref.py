"""float64 numpy restatement of the device augmentation (multitask_hydranet_amd/augment.py docstring, hn_augment.hip): the yardstick of the
kernels.  Every fp32 step is written in numpy float32 in the kernels' operation order; everything else is float64."""
from __future__ import annotations

import math

import numpy as np

MEAN = np.array([0.485, 0.456, 0.406])
STD = np.array([0.229, 0.224, 0.225])
F32 = np.float32


# ---- single geometric ops, written out independently of augment.op_matrix -----------------------------------------------------------
def op_matrix(name, param, W, H):
    cx, cy = W / 2.0, H / 2.0
    T = lambda tx, ty: np.array([[1.0, 0, tx], [0, 1.0, ty], [0, 0, 1.0]])
    if name == "fliplr":
        return np.array([[-1.0, 0, W], [0, 1.0, 0], [0, 0, 1.0]])
    if name == "flipud":
        return np.array([[1.0, 0, 0], [0, -1.0, H], [0, 0, 1.0]])
    if name == "translate_x":
        return T(param, 0)
    if name == "shear_x":
        return T(cx, cy) @ np.array([[1.0, math.tan(math.radians(param)), 0], [0, 1.0, 0], [0, 0, 1.0]]) @ T(-cx, -cy)
    if name == "rotate":
        a = math.radians(param)
        return T(cx, cy) @ np.array([[math.cos(a), -math.sin(a), 0], [math.sin(a), math.cos(a), 0], [0, 0, 1.0]]) @ T(-cx, -cy)
    if name == "crop":
        t, r, b, l = param
        Tp, Rp, Bp, Lp = round(t * H), round(r * W), round(b * H), round(l * W)
        return np.diag([W / (W - Lp - Rp), H / (H - Tp - Bp), 1.0]) @ T(-Lp, -Tp)
    raise ValueError(name)


# ---- Philox4x32-10 ----------------------------------------------------------------------------------------------------------------
def philox4x32_10(ctr, key):
    """ctr: uint32 [..., 4], key: (k0, k1) -> uint32 [..., 4]"""
    c = [np.asarray(ctr[..., i], dtype=np.uint64) for i in range(4)]
    k0, k1 = np.uint64(key[0]), np.uint64(key[1])
    M = np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[0]
        p1 = np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & M, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & M]
        k0 = (k0 + np.uint64(0x9E3779B9)) & M
        k1 = (k1 + np.uint64(0xBB67AE85)) & M
    return np.stack(c, axis=-1).astype(np.uint32)


# ---- photometric ------------------------------------------------------------------------------------------------------------------
def _u8(v):
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def _reflect101(i, n):
    i = np.where(i < 0, -i, i)
    i = np.where(i >= n, 2 * n - 2 - i, i)
    return np.clip(i, 0, n - 1)


def blur(img, radius, w):
    H, W, _ = img.shape
    w = np.asarray(w, dtype=F32)
    x = img.astype(F32)
    acc = np.zeros(img.shape, F32)
    for k in range(-radius, radius + 1):
        acc = acc + w[abs(k)] * x[:, _reflect101(np.arange(W) + k, W)]
    out = np.zeros(img.shape, F32)
    for k in range(-radius, radius + 1):
        out = out + w[abs(k)] * acc[_reflect101(np.arange(H) + k, H)]
    return np.clip(np.rint(out), 0, 255).astype(np.uint8)


def hsv_mul(img, ch, f):
    """OpenCV 8-bit RGB->HSV on the buffer's bytes read as (R, G, B), channel ch times f, float HSV->RGB"""
    x = img.astype(np.int64)
    r, g, b = x[..., 0], x[..., 1], x[..., 2]
    v = np.maximum(np.maximum(r, g), b)
    vmin = np.minimum(np.minimum(r, g), b)
    diff = v - vmin
    sdiv = np.where(v > 0, np.rint((255 << 12) / np.maximum(v, 1).astype(np.float64)), 0).astype(np.int64)
    hdiv = np.where(diff > 0, np.rint((180 << 12) / (6.0 * np.maximum(diff, 1))), 0).astype(np.int64)
    s = (diff * sdiv + (1 << 11)) >> 12
    h = np.where(v == r, g - b, np.where(v == g, b - r + 2 * diff, r - g + 4 * diff))
    h = (h * hdiv + (1 << 11)) >> 12
    h = np.where(h < 0, h + 180, h)
    if ch == 0:
        h = np.rint(h * f).astype(np.int64) % 180
    elif ch == 1:
        s = np.clip(np.rint(s * f), 0, 255).astype(np.int64)
    else:
        v = np.clip(np.rint(v * f), 0, 255).astype(np.int64)
    hf = h.astype(F32)
    sf = s.astype(F32) * F32(1.0 / 255.0)
    vf = v.astype(F32) * F32(1.0 / 255.0)
    hh = hf * F32(F32(6.0) / F32(180.0))
    hh = np.where(hh >= 6, hh - F32(6), hh)
    sector = np.floor(hh).astype(np.int64)
    hh = hh - sector.astype(F32)
    bad = (sector < 0) | (sector >= 6)
    sector = np.where(bad, 0, sector)
    hh = np.where(bad, F32(0), hh).astype(F32)
    tab = np.stack([vf, vf * (F32(1) - sf), vf * (F32(1) - sf * hh), vf * (F32(1) - sf * (F32(1) - hh))], axis=-1)
    sb, sg, sr = np.array([1, 1, 3, 0, 0, 2]), np.array([3, 0, 0, 2, 1, 1]), np.array([0, 2, 1, 1, 3, 0])
    pick = lambda idx: np.take_along_axis(tab, idx[sector][..., None], axis=-1)[..., 0]
    gray = sf == 0
    ro, go, bo = [np.where(gray, vf, pick(t)) for t in (sr, sg, sb)]
    return np.stack([_u8(ro * F32(255)), _u8(go * F32(255)), _u8(bo * F32(255))], axis=-1)


def noise_z(H, W, seed):
    pix = np.arange(H * W, dtype=np.uint64)
    ctr = np.zeros((H * W, 4), dtype=np.uint32)
    ctr[:, 0] = (pix & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    ctr[:, 1] = (pix >> np.uint64(32)).astype(np.uint32)
    w = philox4x32_10(ctr, (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)).astype(np.float64)
    two32 = 4294967296.0
    r0 = np.sqrt(-2.0 * np.log((w[:, 0] + 1.0) / two32))
    r1 = np.sqrt(-2.0 * np.log((w[:, 2] + 1.0) / two32))
    t1, t3 = 2 * np.pi * (w[:, 1] / two32), 2 * np.pi * (w[:, 3] / two32)
    return np.stack([r0 * np.cos(t1), r0 * np.sin(t1), r1 * np.cos(t3)], axis=-1).reshape(H, W, 3)


def photometric(img, d):
    """d: augment.describe()'s dict"""
    op = d["op"]
    if op == 0:
        return img
    x = img.astype(np.float64)
    if op == 1:
        return blur(img, d["radius"], d["w"])
    if op == 2:
        return _u8(127.5 + d["p"][0] * (x - 127.5))
    if op == 3:
        return _u8(x * np.asarray(d["p"][:3]))
    if op == 4:
        z = noise_z(img.shape[0], img.shape[1], d["seed"])
        if not d["per_channel"]:
            z = np.repeat(z[..., :1], 3, axis=-1)
        return _u8(x + d["p"][0] * z)
    return hsv_mul(img, op - 5, d["p"][0])


# ---- warp -------------------------------------------------------------------------------------------------------------------------
def warp_map(finv, H, W):
    """source coordinates of every augmented-frame pixel centre"""
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64) + 0.5, np.arange(W, dtype=np.float64) + 0.5, indexing="ij")
    return finv[0] * xx + finv[1] * yy + finv[2], finv[3] * xx + finv[4] * yy + finv[5]


def warp(img, finv):
    """the intermediate frame: bilinear in pixel-centre space, zero fill, rint + clamp"""
    H, W, _ = img.shape
    px, py = warp_map(finv, H, W)
    u, v = px - 0.5, py - 0.5
    u = np.where(np.isfinite(u), np.clip(u, -4.0, W + 4.0), -4.0)
    v = np.where(np.isfinite(v), np.clip(v, -4.0, H + 4.0), -4.0)
    x0, y0 = np.floor(u), np.floor(v)
    ax, ay = (u - x0)[..., None], (v - y0)[..., None]
    x0, y0 = x0.astype(np.int64), y0.astype(np.int64)

    def tap(yi, xi):
        ok = (xi >= 0) & (xi < W) & (yi >= 0) & (yi < H)
        return np.where(ok[..., None], img[np.clip(yi, 0, H - 1), np.clip(xi, 0, W - 1)].astype(np.float64), 0.0)
    val = (1.0 - ay) * ((1.0 - ax) * tap(y0, x0) + ax * tap(y0, x0 + 1)) + ay * ((1.0 - ax) * tap(y0 + 1, x0) + ax * tap(y0 + 1, x0 + 1))
    return _u8(val)


# ---- INTER_AREA -------------------------------------------------------------------------------------------------------------------
def area_tab(ssize, dsize, scale):
    """computeResizeAreaTab: per output index the list of (source index, fp32 weight)"""
    tab = []
    for dx in range(dsize):
        f1 = dx * scale
        f2 = f1 + scale
        cell = min(scale, ssize - f1)
        s1, s2 = math.ceil(f1), math.floor(f2)
        s2 = min(s2, ssize - 1)
        s1 = min(s1, s2)
        t = []
        if s1 - f1 > 1e-3:
            t.append((s1 - 1, F32((s1 - f1) / cell)))
        for s in range(s1, s2):
            t.append((s, F32(1.0 / cell)))
        if f2 - s2 > 1e-3:
            t.append((s2, F32(min(min(f2 - s2, 1.0), cell) / cell)))
        tab.append(t)
    return tab


def inter_area(img, Hd, Wd):
    Hs, Ws = img.shape[:2]
    if Hs < Hd or Ws < Wd:
        raise ValueError("upscaling")
    sx, sy = 1.0 / (Wd / Ws), 1.0 / (Hd / Hs)
    ix, iy = round(sx), round(sy)
    if abs(sx - ix) < np.finfo(np.float64).eps and abs(sy - iy) < np.finfo(np.float64).eps:
        s = img.reshape(Hd, iy, Wd, ix, -1).astype(np.int64).sum(axis=(1, 3))
        return _u8(s.astype(F32) * (F32(1) / F32(ix * iy)))
    xt, yt = area_tab(Ws, Wd, sx), area_tab(Hs, Hd, sy)
    kx = max(len(t) for t in xt)
    x = img.astype(F32)
    buf = np.zeros((Hs, Wd, img.shape[2]), F32)
    for k in range(kx):                         # per output column: buf = buf + v * alpha in tap order (absent taps add nothing)
        idx = np.array([t[k][0] if k < len(t) else 0 for t in xt])
        a = np.array([t[k][1] if k < len(t) else 0 for t in xt], dtype=F32)
        has = np.array([k < len(t) for t in xt])
        buf = np.where(has[None, :, None], buf + x[:, idx] * a[None, :, None], buf)
    out = np.zeros((Hd, Wd, img.shape[2]), F32)
    ky = max(len(t) for t in yt)
    for k in range(ky):
        idx = np.array([t[k][0] if k < len(t) else 0 for t in yt])
        b = np.array([t[k][1] if k < len(t) else 0 for t in yt], dtype=F32)
        has = np.array([k < len(t) for t in yt])
        out = np.where(has[:, None, None], out + b[:, None, None] * buf[idx], out)
    return _u8(out)


def normalize(rgb_u8):
    """imagenet_normalize of an RGB uint8 image in float64 -> fp32 CHW"""
    return np.transpose((rgb_u8 / np.array([255, 255, 255]) - MEAN) / STD, (2, 0, 1)).astype(np.float32)


def denormalize(chw):
    """the uint8 RGB values behind a normalised fp32 CHW image"""
    return np.rint((np.transpose(chw.astype(np.float64), (1, 2, 0)) * STD + MEAN) * 255.0).astype(np.int64)


def image(frame_bgr, d, Hd, Wd):
    """augment.describe()'s dict d -> (RGB uint8 [Hd, Wd, 3] before normalisation, fp32 CHW)"""
    inter = warp(photometric(frame_bgr, d), d["finv"])
    rgb = inter_area(inter, Hd, Wd)[..., ::-1]
    return rgb, normalize(rgb)


def seg(label, finv, Hd, Wd, tol=1e-4):
    """-> (uint8 [Hd, Wd], alternative candidate, flag of pixels within tol of a floor boundary)"""
    Hs, Ws = label.shape
    ix = np.minimum(np.floor(np.arange(Wd) * (1.0 / (Wd / Ws))).astype(np.int64), Ws - 1)
    iy = np.minimum(np.floor(np.arange(Hd) * (1.0 / (Hd / Hs))).astype(np.int64), Hs - 1)
    cy, cx = np.meshgrid(iy + 0.5, ix + 0.5, indexing="ij")
    px = finv[0] * cx + finv[1] * cy + finv[2]
    py = finv[3] * cx + finv[4] * cy + finv[5]

    def look(qx, qy):
        fx, fy = np.floor(qx), np.floor(qy)
        ok = (fx >= 0) & (fy >= 0) & (fx < Ws) & (fy < Hs)
        return np.where(ok, label[np.clip(fy, 0, Hs - 1).astype(np.int64), np.clip(fx, 0, Ws - 1).astype(np.int64)], 0).astype(np.uint8)
    out = look(px, py)
    near = lambda q: np.abs(q - np.rint(q)) < tol
    flag = near(px) | near(py)
    # the candidates on the other side of a boundary: both coordinates nudged across it
    alts = [look(px + sx * 2 * tol * near(px), py + sy * 2 * tol * near(py)) for sx in (-1, 1) for sy in (-1, 1)]
    return out, alts, flag
