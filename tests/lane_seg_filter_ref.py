"""hn_lane_seg_filter restated in numpy from its contract (include/hydranet_hip.h), not from the kernel: the selection of the
first top_k NMS survivors, the points (x rounded to nearest with ties to even, clamped to +-16383; y = H - 1 - p * interval), a full-frame
boolean mask per lane = the union of its segments under the project's integer thick-line rule, the two counts and the fp32 decision."""
import numpy as np

LIM = 16383


def segment_mask(x0, y0, x1, y1, t, xs, ys):
    """pixel centres within t / 2 of the segment, in integers: 4 * distance^2 <= t^2 (xs, ys: int64 coordinate grids)"""
    dx, dy = x1 - x0, y1 - y0
    len2 = dx * dx + dy * dy
    px, py = xs - x0, ys - y0
    lim = (t * t) >> 2
    to_start = px * px + py * py <= lim
    if len2 == 0:
        return to_start
    dot = px * dx + py * dy
    to_end = (xs - x1) ** 2 + (ys - y1) ** 2 <= lim
    cross = px * dy - py * dx
    to_line = cross * cross <= ((t * t * len2) >> 2)
    return np.where(dot <= 0, to_start, np.where(dot >= len2, to_end, to_line))


def lane_points(xrow, s, e, H, interval):
    """the integer points of one candidate, or None when it paints nothing (fewer than two points, a non-finite x)"""
    if e - s < 2:
        return None
    x = np.asarray(xrow[s:e], np.float32)
    if not np.all(np.isfinite(x)):
        return None
    xi = np.clip(np.rint(x.astype(np.float64)), -LIM, LIM).astype(np.int64)
    return [(int(xi[k]), int(H - 1 - (s + k) * interval)) for k in range(e - s)]


def lane_mask(pts, H, W, t):
    """the union of the segments (p_i, p_{i+1}) over the H x W frame"""
    ys, xs = np.mgrid[0:H, 0:W].astype(np.int64)
    m = np.zeros((H, W), bool)
    for (x0, y0), (x1, y1) in zip(pts, pts[1:]):
        m |= segment_mask(x0, y0, x1, y1, int(t), xs, ys)
    return m


def decide(inter, area, min_ratio):
    with np.errstate(divide="ignore", invalid="ignore"):
        return bool(np.float32(inter) / np.float32(area) > np.float32(min_ratio))


def seg_filter(X, start, end, order, keep, counts, W, H, stride, ppl, interval, mask, lane_class, line_width, min_ratio, top_k):
    """X [N, hw, ppl] fp32; start / end / order / keep [N, hw]; counts [N]; mask int64 [N, H, W] -> keep_out int32 [N, hw],
    stats int32 [N, top_k, 4] = {j, area, inter, kept}, n_sel int32 [N]"""
    N, hw = keep.shape
    assert hw == (W // stride) * (H // stride) and X.shape == (N, hw, ppl) and mask.shape == (N, H, W)
    keep_out = np.zeros((N, hw), np.int32)
    stats = np.zeros((N, top_k, 4), np.int32)
    n_sel = np.zeros(N, np.int32)
    for n in range(N):
        sel = [j for j in range(int(counts[n])) if keep[n, j] != 0][:top_k]
        n_sel[n] = len(sel)
        for k, j in enumerate(sel):
            a = int(order[n, j])
            pts = lane_points(X[n, a], int(start[n, a]), int(end[n, a]), H, interval)
            area = inter = 0
            if pts is not None:
                m = lane_mask(pts, H, W, line_width)
                area = int(m.sum())
                inter = int((m & (mask[n] == lane_class)).sum())
            kept = decide(inter, area, min_ratio)
            stats[n, k] = (j, area, inter, int(kept))
            keep_out[n, j] = int(kept)
    return keep_out, stats, n_sel


def filter_lanes(lanes, mask, H, W, f):
    """the same on one image's decoded Lane objects (descending score, as decode returns them) -> (surviving lanes, stats dicts)"""
    out, stats = [], []
    for ln in lanes[:f.top_k]:
        xs = np.array([p.x for p in ln.lane], np.float32)
        area = inter = 0
        if len(xs) >= 2 and np.all(np.isfinite(xs)):
            xi = np.clip(np.rint(xs.astype(np.float64)), -LIM, LIM).astype(np.int64)
            pts = [(int(x), int(p.y)) for x, p in zip(xi, ln.lane)]
            assert all(float(p.y) == float(q[1]) for p, q in zip(ln.lane, pts))
            m = lane_mask(pts, H, W, f.line_width)
            area, inter = int(m.sum()), int((m & (mask == f.lane_class)).sum())
        kept = decide(inter, area, f.min_ratio)
        stats.append({"score": float(ln.prob), "area": area, "overlap": inter, "kept": kept})
        if kept:
            out.append(ln)
    return out, stats
