// Lane ground-truth encoding (head_lane/lane_codec.py LaneCodec.encode_lane + the dataset's scale-invariance division,
// dataset/dataloader.py:343-352) for a whole batch of packed lane polylines, on device, no host synchronisation.  The host
// (lane_codec.py) parses the annotations: per lane the points scaled to the network input, deduplicated on y, y descending.
//
// Parity rules (every discrete decision below is an exact comparison or an int() truncation of an fp64 value, so the
// arithmetic is IEEE fp64 in the reference's operation order and FMA contraction is off for the whole file):
//   * chord-length natural cubic through the lane's points (lane_spline_interp.py calc_params: the tridiagonal sweep as written there),
//     sampled at t = 0, 1, ... < h per segment, then the last input point; x(t) = a + b*t + (c*t)*t + ((d*t)*t)*t left to right.
//   * the samples are filtered while streaming against the last KEPT one: the first is kept, a later one is dropped when
//     pre_y - y < 1 or it is not strictly inside (0, W) x (0, H); the kept list is reversed (top first).
//   * with interpolate: linear extension from the two last kept points in steps of interval until y >= H - 1.  Lanes spanning < 5 px in y
//     are dropped.  The x(y) fit is FITPACK splrep(s=0): k=1 (piecewise linear) under 4 points, else the not-a-knot cubic interpolant
//     (solved here for the slopes, de Boor's tridiagonal form), evaluated as splev with ext=0 (end pieces extrapolate) at
//     y = H - 1 - k*interval, k = startpos..endpos; an x of exactly 0 becomes 0.01.
//   * anchors in sample order: h = fh - 1 - int(k*interval/stride), w = int(x/stride) (truncation toward zero); out-of-range, already
//     taken by this lane and curr_y <= anchor_y are skipped.  Per anchor the candidate of smallest signed x - W/2 wins (the first in
//     lane order on an exact tie); its loc row is rebuilt from that lane's samples in the reference's write order (up part, up count,
//     down part at descending indices with an exact-0 offset as 1e-6, down count), rounded to fp32, then divided by the interval in fp32.
//
// Kernels:
//   lane_fit_kernel     one workgroup (one wave) per lane: the spline sweep, the streamed samples and the filter, the extension and the
//                       not-a-knot solve on lane 0 of the wave; the evaluation at the P sample heights across the wave; then the lane's
//                       anchor claims (sample index per anchor, -1 = none) into its own map in the workspace.
//   lane_anchor_kernel  one thread per (image, anchor): the winner over the image's lanes and the whole output row, background included.
#include "hn_common.h"

#pragma clang fp contract(off)

#define LE_THREADS 64

struct LaneGeom {
    int W, H, stride, P, fw, fh, F, kc, sc, interpolate, scale_inv;
    double interval;
    float div;
};

__host__ __device__ static inline long le_align(long b) { return (b + 255) & ~255L; }

// workspace carve-up (identical on host and device)
struct LaneWs {
    double* seg;     // [n_points][6] h, C, Dx, Dy, Mx, My of the chord spline
    double* kept;    // [L][kc][2] kept points (x, y), then the fit's extension
    double* fit;     // [L][kc][2] Thomas sweep (c', r' -> slopes)
    double* xs;      // [L][sc] x at the sample heights
    int* hdr;        // [L][4] valid, startpos, endpos
    int* claim;      // [L][F] sample index claiming the anchor, -1 none
};

__host__ __device__ static inline long le_layout(char* base, long n_points, int L, const LaneGeom& g, LaneWs* w) {
    long o = 0;
    const long np = n_points > 0 ? n_points : 1, nl = L > 0 ? L : 1;
    if (w) w->seg = reinterpret_cast<double*>(base + o);
    o += le_align(np * 6 * 8);
    if (w) w->kept = reinterpret_cast<double*>(base + o);
    o += le_align(nl * g.kc * 2 * 8);
    if (w) w->fit = reinterpret_cast<double*>(base + o);
    o += le_align(nl * g.kc * 2 * 8);
    if (w) w->xs = reinterpret_cast<double*>(base + o);
    o += le_align(nl * g.sc * 8);
    if (w) w->hdr = reinterpret_cast<int*>(base + o);
    o += le_align(nl * 4 * 4);
    if (w) w->claim = reinterpret_cast<int*>(base + o);
    o += le_align(nl * (long)g.F * 4);
    return o;
}

static inline LaneGeom le_geom(int W, int H, int stride, int P, int interpolate, int scale_inv, float div) {
    LaneGeom g;
    g.W = W; g.H = H; g.stride = stride; g.P = P;
    g.fw = (int)((double)W / stride);
    g.fh = (int)((double)H / stride);
    g.F = g.fw * g.fh;
    // kept points: the first + at most H strictly inside (0, H) one pixel apart; the extension adds at most P + 2 (interval = H / P)
    g.kc = H + P + 8;
    // samples: endpos - startpos + 1 <= P - startpos, startpos >= -(P + 1) (the host rejects lanes further below the image)
    g.sc = 2 * P + 4;
    g.interpolate = interpolate; g.scale_inv = scale_inv;
    g.interval = (double)H / P;
    g.div = div;
    return g;
}

// the not-a-knot fit of x(y) on ys ascending (m >= 2), evaluated at v
__device__ __forceinline__ double le_eval(const double* kp, const double* s, int m, double v) {
    int lo = 0, hi = m - 1;                          // largest j with ys[j] <= v, clamped to [0, m - 2]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (kp[2 * mid + 1] <= v) lo = mid; else hi = mid;
    }
    const int j = lo;
    const double x0 = kp[2 * j], y0 = kp[2 * j + 1], x1 = kp[2 * j + 2], y1 = kp[2 * j + 3];
    if (m < 4) {
        const double f = 1.0 / (y1 - y0);
        return x0 * (f * (y1 - v)) + x1 * (f * (v - y0));
    }
    const double h = y1 - y0, d = (x1 - x0) / h, s0 = s[2 * j + 1], s1 = s[2 * j + 3];
    const double t = v - y0;
    const double c2 = (3 * d - 2 * s0 - s1) / h;
    const double c3 = (s0 + s1 - 2 * d) / (h * h);
    return x0 + t * (s0 + t * (c2 + t * c3));
}

__global__ void __launch_bounds__(LE_THREADS) lane_fit_kernel(const double* __restrict__ pts, const int* __restrict__ lane_off, LaneGeom g,
                                                               LaneWs ws) {
    const int l = blockIdx.x, tid = threadIdx.x;
    int* claim = ws.claim + (long)l * g.F;
    for (int f = tid; f < g.F; f += LE_THREADS) claim[f] = -1;
    double* kp = ws.kept + (long)l * g.kc * 2;
    double* fit = ws.fit + (long)l * g.kc * 2;
    double* xs = ws.xs + (long)l * g.sc;
    __shared__ int s_m, s_start, s_end, s_valid;
    const double H1 = (double)(g.H - 1);

    if (tid == 0) {
        const int p0 = lane_off[l], n = lane_off[l + 1] - p0;
        const double* x = pts + 2L * p0;             // (x, y) pairs
        double* sg = ws.seg + 6L * p0;
        // calc_params: chord lengths, the forward sweep (C, Dx, Dy), the back substitution (Mx, My)
        for (int i = 0; i < n - 1; ++i) {
            const double dx = x[2 * i] - x[2 * i + 2], dy = x[2 * i + 1] - x[2 * i + 3];
            sg[6 * i] = sqrt(dx * dx + dy * dy);
            sg[6 * i + 4] = 0.0;
            sg[6 * i + 5] = 0.0;
        }
        sg[6 * (n - 1) + 4] = 0.0;
        sg[6 * (n - 1) + 5] = 0.0;
        if (n >= 3) {
            for (int i = 0; i < n - 2; ++i) {
                const double hi = sg[6 * i], hn = sg[6 * i + 6];
                const double A = hi, B = 2 * (hi + hn), Cc = hn;
                const double dx1 = (x[2 * i + 2] - x[2 * i]) / hi, dx2 = (x[2 * i + 4] - x[2 * i + 2]) / hn;
                const double tmpx = 6 * (dx2 - dx1);
                const double dy1 = (x[2 * i + 3] - x[2 * i + 1]) / hi, dy2 = (x[2 * i + 5] - x[2 * i + 3]) / hn;
                const double tmpy = 6 * (dy2 - dy1);
                if (i == 0) {
                    sg[1] = Cc / B;
                    sg[2] = tmpx / B;
                    sg[3] = tmpy / B;
                } else {
                    const double base = B - A * sg[6 * (i - 1) + 1];
                    sg[6 * i + 1] = Cc / base;
                    sg[6 * i + 2] = (tmpx - A * sg[6 * (i - 1) + 2]) / base;
                    sg[6 * i + 3] = (tmpy - A * sg[6 * (i - 1) + 3]) / base;
                }
            }
            sg[6 * (n - 2) + 4] = sg[6 * (n - 3) + 2];
            sg[6 * (n - 2) + 5] = sg[6 * (n - 3) + 3];
            for (int i = n - 4; i >= 0; --i) {
                sg[6 * (i + 1) + 4] = sg[6 * i + 2] - sg[6 * i + 1] * sg[6 * (i + 2) + 4];
                sg[6 * (i + 1) + 5] = sg[6 * i + 3] - sg[6 * i + 1] * sg[6 * (i + 2) + 5];
            }
            sg[4] = sg[5] = 0.0;
            sg[6 * (n - 1) + 4] = sg[6 * (n - 1) + 5] = 0.0;
        }
        // the step-1 samples, filtered while streaming (bottom first)
        int m = 0;
        double pre_y = 0.0;
        auto feed = [&](double cx, double cy) {
            if (m == 0) {
                pre_y = cy;
            } else {
                if (pre_y - cy < 1) return;
                if (!(0 < cx && cx < g.W && 0 < cy && cy < g.H)) return;
                if (m >= g.kc) return;               // (unreachable: see kc)
                pre_y = cy;
            }
            kp[2 * m] = cx;
            kp[2 * m + 1] = cy;
            ++m;
        };
        for (int i = 0; i < n - 1; ++i) {
            const double h = sg[6 * i], M0x = sg[6 * i + 4], M1x = sg[6 * i + 10], M0y = sg[6 * i + 5], M1y = sg[6 * i + 11];
            const double ax = x[2 * i], ay = x[2 * i + 1];
            const double bx = (x[2 * i + 2] - x[2 * i]) / h - (2 * h * M0x + h * M1x) / 6;
            const double by = (x[2 * i + 3] - x[2 * i + 1]) / h - (2 * h * M0y + h * M1y) / 6;
            const double cx = M0x / 2, cy = M0y / 2;
            const double dx = (M1x - M0x) / (6 * h), dy = (M1y - M0y) / (6 * h);
            for (double t = 0; t < h; t += 1)
                feed(ax + bx * t + cx * t * t + dx * t * t * t, ay + by * t + cy * t * t + dy * t * t * t);
        }
        feed(x[2 * (n - 1)], x[2 * (n - 1) + 1]);
        s_m = m;
    }
    __syncthreads();
    {
        const int m = s_m;                           // reverse: y ascending
        for (int i = tid; i < m / 2; i += LE_THREADS) {
            const double ax = kp[2 * i], ay = kp[2 * i + 1];
            kp[2 * i] = kp[2 * (m - 1 - i)];
            kp[2 * i + 1] = kp[2 * (m - 1 - i) + 1];
            kp[2 * (m - 1 - i)] = ax;
            kp[2 * (m - 1 - i) + 1] = ay;
        }
    }
    __syncthreads();
    if (tid == 0) {
        int m = s_m, valid = m >= 2, start = -1, end = -1;
        if (valid && g.interpolate && kp[2 * m - 1] < H1) {
            const double x1 = kp[2 * m - 4], y1 = kp[2 * m - 3], x2 = kp[2 * m - 2], y2 = kp[2 * m - 1];
            double my = y2;
            while (my < H1 && m < g.kc) {
                const double yn = my + g.interval;
                kp[2 * m] = x1 + (x2 - x1) * (yn - y1) / (y2 - y1);
                kp[2 * m + 1] = yn;
                ++m;
                my = yn;
            }
        }
        if (valid && kp[2 * m - 1] - kp[1] < 5) valid = 0;
        if (valid) {
            start = g.interpolate ? 0 : (int)((H1 - kp[2 * m - 1]) / g.interval + 1);
            end = (int)((H1 - kp[1]) / g.interval);
            if (end > g.P - 1) end = g.P - 1;
            if (start >= end) valid = 0;
        }
        if (valid && m >= 4) {
            // not-a-knot slopes: rows {h1, h0 + h1 | r0}, {h_i, 2 (h_{i-1} + h_i), h_{i-1} | r_i}, {h_{m-2} + h_{m-3}, h_{m-3} | r_{m-1}}
            auto yk = [&](int i) { return kp[2 * i + 1]; };
            auto hh = [&](int i) { return yk(i + 1) - yk(i); };
            auto dd = [&](int i) { return (kp[2 * i + 2] - kp[2 * i]) / hh(i); };
            const double h0 = hh(0), h1 = hh(1);
            double cp = (h0 + h1) / h1;
            double rp = (((h0 + 2 * (h0 + h1)) * h1 * dd(0) + h0 * h0 * dd(1)) / (h0 + h1)) / h1;
            fit[0] = cp;
            fit[1] = rp;
            for (int i = 1; i < m; ++i) {
                double lo, di, up, r;
                if (i < m - 1) {
                    const double ha = hh(i - 1), hb = hh(i);
                    lo = hb; di = 2 * (ha + hb); up = ha;
                    r = 3 * (hb * dd(i - 1) + ha * dd(i));
                } else {
                    const double ha = hh(m - 3), hb = hh(m - 2);
                    lo = hb + ha; di = ha; up = 0.0;
                    r = (hb * hb * dd(m - 3) + (2 * (ha + hb) + hb) * ha * dd(m - 2)) / (ha + hb);
                }
                const double den = di - lo * cp;
                cp = up / den;
                rp = (r - lo * rp) / den;
                fit[2 * i] = cp;
                fit[2 * i + 1] = rp;
            }
            for (int i = m - 2; i >= 0; --i) fit[2 * i + 1] = fit[2 * i + 1] - fit[2 * i] * fit[2 * i + 3];
        }
        int* hd = ws.hdr + 4L * l;
        hd[0] = valid; hd[1] = start; hd[2] = end; hd[3] = m;
        s_m = m; s_valid = valid; s_start = start; s_end = end;
    }
    __syncthreads();
    if (!s_valid) return;
    const int m = s_m, start = s_start, len = s_end - s_start + 1;
    for (int i = tid; i < len; i += LE_THREADS) {
        const double v = H1 - (start + i) * g.interval;
        double xv = le_eval(kp, fit, m, v);
        if (xv == 0) xv += 0.01;
        xs[i] = xv;
    }
    __syncthreads();
    if (tid == 0) {
        for (int i = 0; i < len; ++i) {
            const int k = start + i;
            const int h = g.fh - 1 - (int)(k * g.interval / g.stride);
            const double wq = xs[i] / g.stride;
            if (!(fabs(wq) < 1e9)) continue;
            const int w = (int)wq;
            if (h < 0 || h > g.fh - 1 || w < 0 || w > g.fw - 1) continue;
            if (claim[h * g.fw + w] >= 0) continue;
            const double anchor_y = (1.0 * h + 0.5) * g.stride;
            const double curr_y = H1 - k * g.interval;
            if (curr_y <= anchor_y) continue;
            claim[h * g.fw + w] = i;
        }
    }
}

__global__ void __launch_bounds__(256) lane_anchor_kernel(const int* __restrict__ img_lane, int N, LaneGeom g, LaneWs ws,
                                                         float* __restrict__ gt_cls, float* __restrict__ gt_loc) {
    const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= (long)N * g.F) return;
    const int n = (int)(gid / g.F), f = (int)(gid % g.F);
    const int P = g.P, R = 2 * P + 2;
    const double half_w = g.W / 2.0;
    int best = -1, bi = -1;
    double bd = 0.0;
    for (int l = img_lane[n]; l < img_lane[n + 1]; ++l) {
        const int i = ws.claim[(long)l * g.F + f];
        if (i < 0) continue;
        const double d = ws.xs[(long)l * g.sc + i] - half_w;
        if (best < 0 || d < bd) { best = l; bi = i; bd = d; }
    }
    float* row = gt_loc + gid * R;
    gt_cls[2 * gid] = best < 0 ? 1.0f : 0.0f;
    gt_cls[2 * gid + 1] = best < 0 ? 0.0f : 1.0f;
    for (int c = 0; c < R; ++c) row[c] = 0.0f;
    if (best < 0) return;
    const int* hd = ws.hdr + 4L * best;
    const int start = hd[1], len = hd[2] - hd[1] + 1;
    const double* xs = ws.xs + (long)best * g.sc;
    const int h = f / g.fw, w = f % g.fw;
    const double H1 = (double)(g.H - 1);
    const double cx = (1.0 * w + 0.5) * g.stride;
    const double cy = H1 - (double)((g.fh - 1 - h) * (g.P / g.fh)) * g.interval;
    int up = 0;
    for (int j = 0; j < len; ++j) {
        if (H1 - (start + j) * g.interval <= cy) {
            const int c = P + 2 + up;
            if (c < R) row[c] = (float)(xs[j] - cx);
            ++up;
        }
    }
    row[P + 1] = (float)up;
    int di = len - up - 1, dn = 0;
    for (int j = 0; j < len; ++j) {
        if (H1 - (start + j) * g.interval > cy) {
            const double v = xs[j] - cx;
            if (di >= 0 && di < R) row[di] = v == 0 ? (float)0.000001 : (float)v;
            ++dn;
            --di;
        }
    }
    row[P] = (float)dn;
    if (g.scale_inv) {
        for (int c = 0; c < P; ++c) row[c] = row[c] / g.div;
        for (int c = P + 2; c < R; ++c) row[c] = row[c] / g.div;
    }
}

extern "C" long hn_lane_encode_ws_bytes(int n_lanes, long n_points, int W, int H, int stride, int P) {
    if (n_lanes < 0 || n_points < 0 || W < 1 || H < 1 || stride < 1 || P < 1) return -1;
    const LaneGeom g = le_geom(W, H, stride, P, 0, 0, 1.0f);
    return le_layout(nullptr, n_points, n_lanes, g, nullptr);
}

extern "C" int hn_lane_encode(const double* pts, const int* lane_off, const int* img_lane, int N, int n_lanes, long n_points, int W, int H,
                              int stride, int P, int interpolate, int scale_invariance, float div_interval, void* ws, float* gt_cls,
                              float* gt_loc, hipStream_t stream) {
    HN_CHECK_ARG(N >= 1 && n_lanes >= 0 && n_points >= 0 && W >= 1 && H >= 1 && stride >= 1 && P >= 1);
    HN_CHECK_ARG(W / stride >= 1 && H / stride >= 1 && (!scale_invariance || div_interval > 0.0f));
    HN_CHECK_ARG(img_lane && ws && gt_cls && gt_loc && (n_lanes == 0 || (pts && lane_off)));
    const LaneGeom g = le_geom(W, H, stride, P, interpolate ? 1 : 0, scale_invariance ? 1 : 0, div_interval);
    LaneWs w;
    le_layout(static_cast<char*>(ws), n_points, n_lanes, g, &w);
    if (n_lanes > 0) lane_fit_kernel<<<n_lanes, LE_THREADS, 0, stream>>>(pts, lane_off, g, w);
    const long total = (long)N * g.F;
    lane_anchor_kernel<<<(unsigned)((total + 255) / 256), 256, 0, stream>>>(img_lane, N, g, w, gt_cls, gt_loc);
    HN_LAUNCH_CHECK();
}
