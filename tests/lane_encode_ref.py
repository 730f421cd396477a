"""fp64 restatement of lane ground-truth encoding (LaneCodec.encode_lane followed by the dataset's scale-invariance division), written
from the contract in DESIGN.md section 4e with plain Python floats (IEEE fp64, no fused multiply-add) and its own not-a-knot solve, no scipy.

    parse_lanes(lane_object, W, H, org_w, org_h) -> list of (x, y) fp64 arrays per kept lane, y descending (the packer's contract)
    encode_ref(lanes, W, H, stride, P, interpolate, scale_invariance=None, div_interval=None) -> gt_cls fp32 [F, 2], gt_loc fp32 [F, 2P+2]
        (with scale_invariance None the loc rows are returned before the division, as encode_lane returns them)"""
import json
import math

import numpy as np


def parse_lanes(lane_object, W, H, org_w, org_h):
    if isinstance(lane_object, (str, bytes)):
        lane_object = json.loads(lane_object)
    sx, sy = W * 1.0 / org_w, H * 1.0 / org_h
    out = []
    for line in lane_object["Lines"]:
        seen, pts = [], []
        for p in line:
            if p["x"] == "nan" or p["y"] == "nan":
                continue
            if p["y"] in seen:                      # the RAW value: "10" and "10.0" are two points here
                continue
            seen.append(p["y"])
            pts.append((float(p["x"]) * sx, float(p["y"]) * sy))
        if len(pts) < 2:
            continue
        if pts[0][1] < pts[1][1]:
            pts = pts[::-1]
        # ascending float y, the x of the first occurrence of every y, then bottom first
        ys = sorted(set(q[1] for q in pts))
        if len(ys) < 2:
            continue
        first = {}
        for q in pts:
            first.setdefault(q[1], q[0])
        ys = ys[::-1]
        out.append((np.array([first[y] for y in ys], np.float64), np.array(ys, np.float64)))
    return out


def _natural_params(x, y):
    """chord-length natural cubic (second derivatives M over chord parameter), the tridiagonal sweep in its textbook order"""
    n = len(x)
    h = [math.sqrt((x[i] - x[i + 1]) * (x[i] - x[i + 1]) + (y[i] - y[i + 1]) * (y[i] - y[i + 1])) for i in range(n - 1)]
    mx, my = [0.0] * n, [0.0] * n
    if n >= 3:
        c, dx, dy = [], [], []
        for i in range(n - 2):
            a, b, cc = h[i], 2 * (h[i] + h[i + 1]), h[i + 1]
            tx = 6 * ((x[i + 2] - x[i + 1]) / h[i + 1] - (x[i + 1] - x[i]) / h[i])
            ty = 6 * ((y[i + 2] - y[i + 1]) / h[i + 1] - (y[i + 1] - y[i]) / h[i])
            if i == 0:
                c.append(cc / b)
                dx.append(tx / b)
                dy.append(ty / b)
            else:
                base = b - a * c[i - 1]
                c.append(cc / base)
                dx.append((tx - a * dx[i - 1]) / base)
                dy.append((ty - a * dy[i - 1]) / base)
        mx[n - 2], my[n - 2] = dx[n - 3], dy[n - 3]
        for i in range(n - 4, -1, -1):
            mx[i + 1] = dx[i] - c[i] * mx[i + 2]
            my[i + 1] = dy[i] - c[i] * my[i + 2]
        mx[0] = mx[n - 1] = my[0] = my[n - 1] = 0.0
    segs = []
    for i in range(n - 1):
        bx = (x[i + 1] - x[i]) / h[i] - (2 * h[i] * mx[i] + h[i] * mx[i + 1]) / 6
        by = (y[i + 1] - y[i]) / h[i] - (2 * h[i] * my[i] + h[i] * my[i + 1]) / 6
        segs.append((x[i], bx, mx[i] / 2, (mx[i + 1] - mx[i]) / (6 * h[i]),
                     y[i], by, my[i] / 2, (my[i + 1] - my[i]) / (6 * h[i]), h[i]))
    return segs


def _densify_filter(x, y, W, H):
    """step-1 samples of every chord segment plus the last input point, filtered against the last KEPT point; returned top first"""
    kx, ky = [], []
    pre_y = None

    def feed(cx, cy):
        nonlocal pre_y
        if pre_y is None:
            pre_y = cy
            kx.append(cx)
            ky.append(cy)
            return
        if pre_y - cy < 1:
            return
        if not (0 < cx < W and 0 < cy < H):
            return
        kx.append(cx)
        ky.append(cy)
        pre_y = cy

    for ax, bx, cx, dx, ay, by, cy, dy, h in _natural_params([float(v) for v in x], [float(v) for v in y]):
        t = 0
        while t < h:
            feed(ax + bx * t + cx * t * t + dx * t * t * t, ay + by * t + cy * t * t + dy * t * t * t)
            t += 1
    feed(float(x[-1]), float(y[-1]))
    return kx[::-1], ky[::-1]


def _fit_eval(ys, xs, q):
    """FITPACK splrep(ys, xs, s=0) + splev(q, ext=0): k=1 under 4 points, else the not-a-knot cubic interpolant (end pieces extrapolate)"""
    m = len(ys)
    idx = np.clip(np.searchsorted(ys, q, side="right") - 1, 0, m - 2)
    out = []
    if m < 4:
        for v, j in zip(q, idx):
            f = 1.0 / (ys[j + 1] - ys[j])
            out.append(xs[j] * (f * (ys[j + 1] - v)) + xs[j + 1] * (f * (v - ys[j])))
        return out
    h = [ys[i + 1] - ys[i] for i in range(m - 1)]
    d = [(xs[i + 1] - xs[i]) / h[i] for i in range(m - 1)]
    # slopes s: not-a-knot end rows, the standard interior rows; Thomas sweep
    lo, di, up, r = [0.0] * m, [0.0] * m, [0.0] * m, [0.0] * m
    di[0], up[0] = h[1], h[0] + h[1]
    r[0] = ((h[0] + 2 * (h[0] + h[1])) * h[1] * d[0] + h[0] * h[0] * d[1]) / (h[0] + h[1])
    for i in range(1, m - 1):
        lo[i], di[i], up[i] = h[i], 2 * (h[i - 1] + h[i]), h[i - 1]
        r[i] = 3 * (h[i] * d[i - 1] + h[i - 1] * d[i])
    lo[m - 1], di[m - 1] = h[m - 2] + h[m - 3], h[m - 3]
    r[m - 1] = (h[m - 2] * h[m - 2] * d[m - 3] + (2 * (h[m - 3] + h[m - 2]) + h[m - 2]) * h[m - 3] * d[m - 2]) / (h[m - 3] + h[m - 2])
    cp, rp = [0.0] * m, [0.0] * m
    cp[0], rp[0] = up[0] / di[0], r[0] / di[0]
    for i in range(1, m):
        den = di[i] - lo[i] * cp[i - 1]
        cp[i] = up[i] / den
        rp[i] = (r[i] - lo[i] * rp[i - 1]) / den
    s = [0.0] * m
    s[m - 1] = rp[m - 1]
    for i in range(m - 2, -1, -1):
        s[i] = rp[i] - cp[i] * s[i + 1]
    for v, j in zip(q, idx):
        t = v - ys[j]
        c2 = (3 * d[j] - 2 * s[j] - s[j + 1]) / h[j]
        c3 = (s[j] + s[j + 1] - 2 * d[j]) / (h[j] * h[j])
        out.append(xs[j] + t * (s[j] + t * (c2 + t * c3)))
    return out


def _sample_lane(kx, ky, W, H, P, interval, interpolate):
    if len(kx) < 2:
        return None
    kx, ky = list(kx), list(ky)
    if interpolate and ky[-1] < H - 1:
        x1, y1, x2, y2 = kx[-2], ky[-2], kx[-1], ky[-1]
        my = ky[-1]
        while my < H - 1:
            yn = my + interval
            kx.append(x1 + (x2 - x1) * (yn - y1) / (y2 - y1))
            ky.append(yn)
            my = yn
    if max(ky) - min(ky) < 5:
        return None
    start = 0 if interpolate else int((H - 1 - ky[-1]) / interval + 1)
    end = min(int((H - 1 - ky[0]) / interval), P - 1)
    if start >= end:
        return None
    q = [H - 1 - i * interval for i in range(start, end + 1)]
    xl = _fit_eval(np.array(ky), np.array(kx), q)
    xl = [0.01 if v == 0 else v for v in xl]
    return start, end, xl


def encode_ref(lanes, W, H, stride, P, interpolate, scale_invariance=None, div_interval=None):
    fw, fh = int(W / stride), int(H / stride)
    interval = float(H) / P
    q = int(P / fh)
    cand = {}                                        # anchor -> [(distance, row)] in lane order
    for x, y in lanes:
        kx, ky = _densify_filter(x, y, W, H)
        smp = _sample_lane(kx, ky, W, H, P, interval, interpolate)
        if smp is None:
            continue
        start, end, xl = smp
        L = end - start + 1
        ylist = [H - 1 - k * interval for k in range(start, end + 1)]
        taken = set()
        for i in range(L):
            h = fh - 1 - int((start + i) * interval / stride)
            w = int(xl[i] / stride)
            if h < 0 or h > fh - 1 or w < 0 or w > fw - 1 or (h, w) in taken:
                continue
            if H - 1 - (i + start) * interval <= (1.0 * h + 0.5) * stride:
                continue
            taken.add((h, w))
            cx = (1.0 * w + 0.5) * stride
            cy = H - 1 - (fh - 1 - h) * q * interval
            row = [0.0] * (2 * P + 2)
            up = 0
            for j in range(L):
                if ylist[j] <= cy:
                    row[P + 2 + up] = xl[j] - cx
                    up += 1
            row[P + 1] = up
            di, dn = L - up - 1, 0
            for j in range(L):
                if ylist[j] > cy:
                    row[di] = 0.000001 if xl[j] - cx == 0 else xl[j] - cx
                    dn += 1
                    di -= 1
            row[P] = dn
            cand.setdefault(h * fw + w, []).append((xl[i] - W / 2, row))
    cls = np.zeros((fw * fh, 2), np.float64)
    cls[:, 0] = 1
    loc = np.zeros((fw * fh, 2 * P + 2), np.float64)
    for f, lst in cand.items():
        best = lst[0]
        for c in lst[1:]:
            if c[0] < best[0]:                       # first candidate in lane order on an exact tie
                best = c
        cls[f] = (0, 1)
        loc[f] = best[1]
    cls, loc = cls.astype(np.float32), loc.astype(np.float32)
    if scale_invariance:
        dv = np.float32(div_interval if div_interval is not None else interval)
        loc[:, P + 2:2 * P + 2] /= dv
        loc[:, :P] /= dv
    return cls, loc
