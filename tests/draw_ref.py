"""multitask_hydranet_amd/draw.py restated in numpy from its specification: the primitive semantics (paint) -- thick segment =
the pixel centres within thickness / 2 of the segment, in integers; filled rectangle with both corners inclusive; 5 x 7 glyph bitmap
scaled by an integer; the LAST primitive of the list that covers a pixel gives its colour -- and the host logic of the two helpers:
lanes -> primitives (lanedetect.py:126-178) and boxes -> primitives (display.py:49-84).  Only the font bitmaps and the colour table are
taken from the module (they are data); the rules are written again here.  Primitive tuples: (kind, x0, y0, x1, y1, param, colour word)."""
import numpy as np

from multitask_hydranet_amd.draw import CLASS_COLORS_BGR, FONT

LIM = 16383


def clampc(v):
    return max(-LIM, min(LIM, int(v)))


def word(c):
    return (int(c[0]) & 255) | ((int(c[1]) & 255) << 8) | ((int(c[2]) & 255) << 16)


def covers(p, xs, ys):
    """bool mask over the int64 coordinate grids xs, ys"""
    kind, x0, y0, x1, y1, param, _ = p
    if kind == 0:
        dx, dy = x1 - x0, y1 - y0
        len2 = dx * dx + dy * dy
        px, py = xs - x0, ys - y0
        dot = px * dx + py * dy
        d_start = px * px + py * py
        d_end = (xs - x1) ** 2 + (ys - y1) ** 2
        cross = (px * dy - py * dx) ** 2
        t2 = param * param
        if len2 == 0:
            return d_start <= (t2 >> 2)
        return np.where(dot <= 0, d_start <= (t2 >> 2), np.where(dot >= len2, d_end <= (t2 >> 2), cross <= ((t2 * len2) >> 2)))
    if kind == 1:
        return (xs >= min(x0, x1)) & (xs <= max(x0, x1)) & (ys >= min(y0, y1)) & (ys <= max(y0, y1))
    lx, ly = xs - x0, ys - y0
    inside = (lx >= 0) & (ly >= 0) & (lx < 5 * param) & (ly < 7 * param)
    cx, cy = np.clip(lx // param, 0, 4), np.clip(ly // param, 0, 6)
    rows = [(x1 >> (5 * r)) & 31 for r in range(4)] + [(y1 >> (5 * r)) & 31 for r in range(3)]
    bits = np.array([[(rows[r] >> (4 - c)) & 1 for c in range(5)] for r in range(7)], dtype=bool)
    return inside & bits[cy, cx]


def paint(frame, prims):
    """a painted copy of the uint8 H x W x 3 frame"""
    out = frame.copy()
    h, w = out.shape[:2]
    ys, xs = np.mgrid[0:h, 0:w].astype(np.int64)
    for p in prims:
        m = covers(p, xs, ys)
        out[m] = (p[6] & 255, (p[6] >> 8) & 255, (p[6] >> 16) & 255)
    return out


# ---- primitives of the two helpers -----------------------------------------------------------------------------------------------------
def seg(a, b, t, colour):
    return (0, clampc(a[0]), clampc(a[1]), clampc(b[0]), clampc(b[1]), max(1, int(t)), word(colour))


def glyphs(x, y, s, string, colour):
    out = []
    for i, ch in enumerate(string):
        rows = FONT.get(ch, (0,) * 7)
        if not any(rows):
            continue
        lo = sum(rows[r] << (5 * r) for r in range(4))
        hi = sum(rows[4 + r] << (5 * r) for r in range(3))
        out.append((2, clampc(int(x) + 6 * s * i), clampc(int(y) - 7 * s), lo, hi, s, word(colour)))
    return out


def lane_prims(lanes, org_width=1920, min_length=2, filter_vertical=True, filter_thres=65):
    import warnings
    out = []
    for ln in lanes:
        pts = [(int(p["x"]), int(p["y"])) for p in ln["points"]]
        if len(pts) < min_length:
            continue
        if filter_vertical:
            a = np.array(pts)
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                slope = np.polyfit(a[:, 0], a[:, 1], 1)[0]
            if abs(np.arctan(slope)) / 3.1415 * 180 > filter_thres:
                continue
        for i in range(len(pts) - 1):
            out.append(seg(pts[i], pts[i + 1], 15, (255, 255, 0)))
        tx, ty = pts[min_length - 1]
        if tx < 0:
            tx = 30
        if tx > org_width:
            tx = org_width - 300
            ty = ty - 60
        out += glyphs(tx, ty - 10, 6, "Lane: %.2f" % float(ln["score"]), (255, 255, 0))      # font scale 2.0 -> 6
    return out


def box_prims(pred, img_hw, obj_list, org_size, target_size):
    out = []
    tl = int(round(0.003 * max(img_hw)))
    t, s = max(1, tl), max(1, int(round(3.0 * (float(tl) / 3))))
    for roi, cid, score in zip(np.asarray(pred["rois"]), pred["class_ids"], pred["scores"]):
        x1, y1, x2, y2 = [int(v) for v in roi]
        c1 = (int(x1 / float(target_size[0]) * org_size[0]), int(y1 / float(target_size[1]) * org_size[1]))
        c2 = (int(x2 / float(target_size[0]) * org_size[0]), int(y2 / float(target_size[1]) * org_size[1]))
        name = obj_list[int(cid)]
        colour = CLASS_COLORS_BGR[obj_list.index(name) % len(CLASS_COLORS_BGR)]
        for a, b in (((c1[0], c1[1]), (c2[0], c1[1])), ((c2[0], c1[1]), (c2[0], c2[1])), ((c2[0], c2[1]), (c1[0], c2[1])), ((c1[0], c2[1]), (c1[0], c1[1]))):
            out.append(seg(a, b, t, colour))
        pct = "{:.0%}".format(float(score))
        out.append((1, clampc(c1[0]), clampc(c1[1]), clampc(c1[0] + 6 * s * len(name) + 6 * s * len(pct) + 15), clampc(c1[1] - 7 * s - 3), 1, word(colour)))
        out += glyphs(c1[0], c1[1] - 2, s, name + pct, (0, 0, 0))
    return out
