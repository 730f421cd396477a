// Lane F1 for a ragged batch of images (head_lane/lane_metric.py:45-209; lane_metric.py LaneIoUBatch): every lane's natural
// cubic spline, its unit-step samples, the thick-line rasterisation and the pixel counts |g & p|, |g|, |p| of every (ground truth,
// prediction) pair, without a full-frame mask in HBM.
//   lane_spline_kernel   one thread per lane: calc_params in float64, operation for operation (chord lengths with a correctly rounded square
//                        root, every + 1e-8 guard, the Thomas sweep and the back substitution in the reference's order, M_0 = M_{n-1} = 0; two
//                        points = the straight line), and the number of samples of every segment (t = 0, 1, 2, ... < h) + 1 for the lane's
//                        own last point.  One entry per POINT: entry k of a lane is the segment that starts at point k, the lane's last entry
//                        is the appended last point.
//   lane_scan_kernel     one workgroup: exclusive prefix sum over all entries of the batch = every sample's slot
//   lane_sample_kernel   one thread per sample: x = ((a + b t) + (c t) t) + ((d t) t) t, likewise y, truncated toward zero (Python's int())
//   lane_tile_kernel     one workgroup per 64 x 64 tile of one image and one block of 32 x 32 pairs: one bit per lane and pixel in LDS, painted
//                        with lane_raster_kernel's integer distance test (hn_post.hip), then counted into the image's uint64 tables with
//                        integer atomics (exact, order independent)
// Every float64 operation rounds once, as numpy's does: contraction of a * b + c into an FMA is off for the whole file.
#include "hn_common.h"
#pragma clang fp contract(off)

#define LM_TILE 64
#define LM_BLOCK 32                      // lanes per side of a pair block (one 32-bit word per side and pixel)
#define LM_MAX_H 1.0e9                   // a longer segment is not sampled (the status word reports it): the host packer refuses such lanes

// exclusive prefix sum over the NT threads of a workgroup (NT a multiple of 64, at most 1024); total: the sum, in every thread
template <int NT>
__device__ __forceinline__ unsigned block_scan(unsigned v, unsigned* s_w, unsigned& total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    unsigned inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned o = __shfl_up(inc, d, 64);
        if (lane >= d) inc += o;
    }
    __syncthreads();                                                     // s_w may still be read from the previous call
    if (lane == 63) s_w[w] = inc;
    __syncthreads();
    unsigned before = 0, all = 0;
#pragma unroll
    for (int i = 0; i < NT / 64; ++i) {
        const unsigned t = s_w[i];
        if (i < w) before += t;
        all += t;
    }
    total = all;
    return before + inc - v;
}

// `t = 0; while t < h: t += 1` runs this many times: the smallest integer n that fails n < h (0 for h <= 0 and for a NaN)
__device__ __forceinline__ unsigned sample_count(double h, int* bad) {
    if (!(0.0 < h)) return 0;
    if (!(h < LM_MAX_H)) { *bad = 1; return 0; }
    unsigned n = (unsigned)h;
    while ((double)n < h) ++n;
    while (n > 0 && !((double)(n - 1) < h)) --n;
    return n;
}

// coef: [n_points][9] = a_x, b_x, c_x, d_x, a_y, b_y, c_y, d_y, h of the segment that starts at the point; scr: 5 arrays of n_points
__global__ __launch_bounds__(64) void lane_spline_kernel(const double* __restrict__ pts, const int* __restrict__ lane_off, int n_lanes, long n_points,
                                                         double* __restrict__ coef, double* __restrict__ scr, unsigned* __restrict__ cnt,
                                                         int* __restrict__ pt_lane, unsigned long long* status) {
    const int l = blockIdx.x * 64 + threadIdx.x;
    if (l >= n_lanes) return;
    const long p0 = lane_off[l], p1 = lane_off[l + 1];
    if (p0 < 0 || p1 < p0 || p1 > n_points) return;                      // (a malformed table paints nothing: cnt is zeroed)
    const int n = (int)(p1 - p0);
    if (n == 0) return;
    for (long k = p0; k < p1; ++k) pt_lane[k] = l;
    cnt[p1 - 1] = 1;                                                     // the lane's own last point
    if (n == 1) return;
    const double* X = pts + 2 * p0;                                      // x_i = X[2 i], y_i = X[2 i + 1]
    double* co = coef + 9 * p0;
    int bad = 0;
    if (n == 2) {
        const double x0 = X[0], y0 = X[1], x1 = X[2], y1 = X[3];
        const double h0 = __dsqrt_rn((x0 - x1) * (x0 - x1) + (y0 - y1) * (y0 - y1));
        co[0] = x0; co[1] = (x1 - x0) / (h0 + 1e-8); co[2] = 0.0; co[3] = 0.0;
        co[4] = y0; co[5] = (y1 - y0) / (h0 + 1e-8); co[6] = 0.0; co[7] = 0.0;
        co[8] = h0;
        cnt[p0] = sample_count(h0, &bad);
        if (bad) *status = 1;
        return;
    }
    double* cs = scr + p0;
    double* dxs = scr + n_points + p0;
    double* dys = scr + 2 * n_points + p0;
    double* mx = scr + 3 * n_points + p0;
    double* my = scr + 4 * n_points + p0;
    for (int i = 0; i < n - 1; ++i) {
        const double dx = X[2 * i] - X[2 * i + 2], dy = X[2 * i + 1] - X[2 * i + 3];
        co[9 * i + 8] = __dsqrt_rn(dx * dx + dy * dy);
    }
#define LM_H(i) co[9 * (i) + 8]
    // Thomas sweep of the tridiagonal system for the second derivatives M_1 .. M_{n-2}
    for (int i = 0; i < n - 2; ++i) {
        const double a = LM_H(i), b = 2.0 * (LM_H(i) + LM_H(i + 1)), c = LM_H(i + 1);
        const double tx = 6.0 * ((X[2 * i + 4] - X[2 * i + 2]) / (LM_H(i + 1) + 1e-8) - (X[2 * i + 2] - X[2 * i]) / (LM_H(i) + 1e-8));
        const double ty = 6.0 * ((X[2 * i + 5] - X[2 * i + 3]) / (LM_H(i + 1) + 1e-8) - (X[2 * i + 3] - X[2 * i + 1]) / (LM_H(i) + 1e-8));
        if (i == 0) {
            cs[0] = c / (b + 1e-8);
            dxs[0] = tx / (b + 1e-8);
            dys[0] = ty / (b + 1e-8);
        } else {
            const double base = b - a * cs[i - 1];
            cs[i] = c / (base + 1e-8);
            dxs[i] = (tx - a * dxs[i - 1]) / (base + 1e-8);
            dys[i] = (ty - a * dys[i - 1]) / (base + 1e-8);
        }
    }
    mx[n - 2] = dxs[n - 3];
    my[n - 2] = dys[n - 3];
    for (int i = n - 4; i >= 0; --i) {
        mx[i + 1] = dxs[i] - cs[i] * mx[i + 2];
        my[i + 1] = dys[i] - cs[i] * my[i + 2];
    }
    mx[0] = mx[n - 1] = my[0] = my[n - 1] = 0.0;
    for (int i = 0; i < n - 1; ++i) {
        const double h = LM_H(i), xi = X[2 * i], yi = X[2 * i + 1], xn = X[2 * i + 2], yn = X[2 * i + 3];
        co[9 * i + 0] = xi;
        co[9 * i + 1] = (xn - xi) / (h + 1e-8) - ((2.0 * h) * mx[i] + h * mx[i + 1]) / 6.0;
        co[9 * i + 2] = mx[i] / 2.0;
        co[9 * i + 3] = (mx[i + 1] - mx[i]) / (6.0 * (h + 1e-8));
        co[9 * i + 4] = yi;
        co[9 * i + 5] = (yn - yi) / (h + 1e-8) - ((2.0 * h) * my[i] + h * my[i + 1]) / 6.0;
        co[9 * i + 6] = my[i] / 2.0;
        co[9 * i + 7] = (my[i + 1] - my[i]) / (6.0 * (h + 1e-8));
        cnt[p0 + i] = sample_count(h, &bad);
    }
#undef LM_H
    if (bad) *status = 1;
}

// off[k] = sum of cnt[0 .. k) in place, off[n_points] = the number of samples; more samples than the caller's buffer holds: status
__global__ __launch_bounds__(1024) void lane_scan_kernel(unsigned* off, long n_points, long sample_cap, unsigned long long* status) {
    __shared__ unsigned s_w[16];
    unsigned long long carry = 0;
    for (long base = 0; base < n_points; base += 1024) {
        const long k = base + threadIdx.x;
        const unsigned v = k < n_points ? off[k] : 0u;
        unsigned total;
        const unsigned ex = block_scan<1024>(v, s_w, total);
        if (k < n_points) off[k] = (unsigned)min(carry + ex, 0xffffffffull);
        carry += total;
    }
    if (threadIdx.x == 0) {
        off[n_points] = (unsigned)min(carry, 0xffffffffull);
        if (carry > (unsigned long long)sample_cap) *status = 2;
    }
}

__device__ __forceinline__ int trunc_i32(double v) {                     // int(): toward zero; saturating outside int32, 0 for a NaN
    if (!(v == v)) return 0;
    if (v >= 2147483647.0) return 2147483647;
    if (v <= -2147483648.0) return -2147483647 - 1;
    return (int)v;
}

// smp: int32 [sample_cap][4] = x, y, lane, 0
__global__ __launch_bounds__(256) void lane_sample_kernel(const double* __restrict__ pts, const int* __restrict__ lane_off, int n_lanes,
                                                          long n_points, const double* __restrict__ coef, const unsigned* __restrict__ off,
                                                          const int* __restrict__ pt_lane, long sample_cap, int4* __restrict__ smp) {
    const long s = (long)blockIdx.x * 256 + threadIdx.x;
    const long total = min((long)off[n_points], sample_cap);
    if (s >= total) return;
    long lo = 0, hi = n_points;                                          // the last entry k with off[k] <= s (the one that holds slot s)
    while (hi - lo > 1) {
        const long mid = (lo + hi) >> 1;
        if ((long)off[mid] <= s) lo = mid; else hi = mid;
    }
    const long k = lo;
    const int l = pt_lane[k];
    int4 o = make_int4(0, 0, -1, 0);
    if (l >= 0 && l < n_lanes) {
        o.z = l;
        if (k == (long)lane_off[l + 1] - 1) {
            o.x = trunc_i32(pts[2 * k]);
            o.y = trunc_i32(pts[2 * k + 1]);
        } else {
            const double* c = coef + 9 * k;
            const double t = (double)(s - (long)off[k]);
            o.x = trunc_i32(((c[0] + c[1] * t) + (c[2] * t) * t) + ((c[3] * t) * t) * t);
            o.y = trunc_i32(((c[4] + c[5] * t) + (c[6] * t) * t) + ((c[7] * t) * t) * t);
        }
    }
    smp[s] = o;
}

struct LaneTabs {                        // the host's packed int32 tables (lane_metric.py pack_lane_batch)
    const int* lane_off;                 // [n_lanes + 1] CSR: the points of every lane
    const int* img_lane;                 // [N + 1] CSR: the lanes of every image, its ground truths first
    const int* img_g;                    // [N] number of ground-truth lanes
    const int* img_h;                    // [N]
    const int* img_w;                    // [N]
    const int* cnt_off;                  // [N] the image's tables in counts: inter [G][P], then area [G + P]
    const int* work;                     // [n_work][4] = image, g0, p0, first tile: one pair block of one image, tiles in raster order
};

__global__ __launch_bounds__(256) void lane_tile_kernel(const int4* __restrict__ smp, const unsigned* __restrict__ off, LaneTabs T, int N, int n_lanes,
                                                        long n_points, int n_work, long n_tiles, long sample_cap, int width2,
                                                        unsigned long long* __restrict__ counts, long n_tables) {
    __shared__ unsigned bits[2][LM_TILE * LM_TILE];                      // [0]: ground truths, [1]: predictions; bit = lane within the block
    __shared__ unsigned cntl[LM_BLOCK * LM_BLOCK + 2 * LM_BLOCK];
    __shared__ int seg[256][5];                                          // x0, y0, x1, y1, side * 32 + bit
    __shared__ int nseg;
    __shared__ unsigned any[2];
    const int tid = threadIdx.x;
    const long tile = blockIdx.x;
    if (tile >= n_tiles) return;
    int lo = 0, hi = n_work;                                             // the last work item whose first tile is <= tile
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if ((long)T.work[4 * mid + 3] <= tile) lo = mid; else hi = mid;
    }
    const int img = T.work[4 * lo], g0 = T.work[4 * lo + 1], p0 = T.work[4 * lo + 2];
    if (img < 0 || img >= N || g0 < 0 || p0 < 0) return;
    const int H = T.img_h[img], W = T.img_w[img];
    const int la = T.img_lane[img], nl = T.img_lane[img + 1] - la, G = T.img_g[img], P = nl - G;
    if (H <= 0 || W <= 0 || la < 0 || nl < 0 || la + nl > n_lanes || G < 0 || P < 0) return;
    const int tiles_x = (W + LM_TILE - 1) / LM_TILE, tiles_y = (H + LM_TILE - 1) / LM_TILE;
    const long lt = tile - T.work[4 * lo + 3];
    if (lt >= (long)tiles_x * tiles_y) return;
    const int X0 = (int)(lt % tiles_x) * LM_TILE, Y0 = (int)(lt / tiles_x) * LM_TILE;
    const int X1 = min(X0 + LM_TILE, W) - 1, Y1 = min(Y0 + LM_TILE, H) - 1;       // the tile's pixels, inside the image
    const int cnt_side[2] = {max(min(LM_BLOCK, G - g0), 0), max(min(LM_BLOCK, P - p0), 0)};
    const int first[2] = {la + g0, la + G + p0};                         // first lane of either side of the block

    for (int i = tid; i < 2 * LM_TILE * LM_TILE; i += 256) (&bits[0][0])[i] = 0;
    for (int i = tid; i < LM_BLOCK * LM_BLOCK + 2 * LM_BLOCK; i += 256) cntl[i] = 0;
    if (tid < 2) any[tid] = 0;
    if (tid == 0) nseg = 0;
    __syncthreads();

    const long total = min((long)off[n_points], sample_cap);
    const long r = (width2 + 3) / 4 + 1;                                 // width2 = 2 * lane_width: radius lane_width / 2, rounded up, + 1
    for (int side = 0; side < 2; ++side) {
        if (cnt_side[side] == 0) continue;
        // the block's lanes of one side are neighbours, so their samples are one range
        const long q0 = T.lane_off[first[side]], q1 = T.lane_off[first[side] + cnt_side[side]];
        if (q0 < 0 || q1 < q0 || q1 > n_points) continue;
        const long s0 = off[q0], s1 = min((long)off[q1], total);
        for (long base = s0; base < s1; base += 256) {
            const long j = base + tid;
            if (j + 1 < s1) {
                const int4 a = smp[j], b = smp[j + 1];
                if (a.z == b.z) {                                        // one lane: a segment of its polyline
                    const long bx0 = max(min((long)a.x, (long)b.x) - r, 0l), bx1 = min(max((long)a.x, (long)b.x) + r, (long)W - 1);
                    const long by0 = max(min((long)a.y, (long)b.y) - r, 0l), by1 = min(max((long)a.y, (long)b.y) + r, (long)H - 1);
                    if (bx0 <= X1 && bx1 >= X0 && by0 <= Y1 && by1 >= Y0) {
                        const int e = atomicAdd(&nseg, 1);
                        seg[e][0] = a.x; seg[e][1] = a.y; seg[e][2] = b.x; seg[e][3] = b.y;
                        seg[e][4] = side * 32 + (a.z - first[side]);
                    }
                }
            }
            __syncthreads();
            const int ns = nseg;
            for (int e = tid >> 6; e < ns; e += 4) {                     // one wave per segment: its box, clipped to the tile
                const long x0 = seg[e][0], y0 = seg[e][1], x1 = seg[e][2], y1 = seg[e][3];
                const int sd = seg[e][4] >> 5;
                const unsigned m = 1u << (seg[e][4] & 31);
                const int bx0 = (int)max(min(x0, x1) - r, (long)X0), bx1 = (int)min(max(x0, x1) + r, (long)X1);
                const int by0 = (int)max(min(y0, y1) - r, (long)Y0), by1 = (int)min(max(y0, y1) + r, (long)Y1);
                const int bw = bx1 - bx0 + 1, n = bw * (by1 - by0 + 1);
                const long dx = x1 - x0, dy = y1 - y0, len2 = dx * dx + dy * dy;
                for (int k = tid & 63; k < n; k += 64) {
                    const int x = bx0 + k % bw, y = by0 + k / bw;
                    unsigned* word = &bits[sd][(y - Y0) * LM_TILE + (x - X0)];
                    if (*word & m) continue;                             // (painted by a neighbour segment already)
                    const long px = x - x0, py = y - y0;
                    // squared distance from (x, y) to the segment, scaled by len2 (integers: exact), as lane_raster_kernel
                    long num, den;
                    const long dot = px * dx + py * dy;
                    if (len2 == 0 || dot <= 0) { num = px * px + py * py; den = 1; }
                    else if (dot >= len2) { const long qx = x - x1, qy = y - y1; num = qx * qx + qy * qy; den = 1; }
                    else { const long cr = px * dy - py * dx; num = cr * cr; den = len2; }
                    if (16 * num <= (long)width2 * width2 * den) atomicOr(word, m);
                }
            }
            __syncthreads();
            if (tid == 0) nseg = 0;
            __syncthreads();
        }
    }

    // count: every thread owns 16 pixels
    unsigned gb[16], pb[16], og = 0, op = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        gb[i] = bits[0][i * 256 + tid];
        pb[i] = bits[1][i * 256 + tid];
        og |= gb[i];
        op |= pb[i];
    }
    if (og) atomicOr(&any[0], og);
    if (op) atomicOr(&any[1], op);
    __syncthreads();
    const unsigned ag = any[0], ap = any[1];
    if (!(ag | ap)) return;
    for (unsigned mg = ag; mg; mg &= mg - 1) {
        const int g = __ffs(mg) - 1;
        unsigned c = 0;
#pragma unroll
        for (int i = 0; i < 16; ++i) c += (gb[i] >> g) & 1u;
        if (c) atomicAdd(&cntl[LM_BLOCK * LM_BLOCK + g], c);
        for (unsigned mp = ap; mp; mp &= mp - 1) {
            const int p = __ffs(mp) - 1;
            unsigned cp = 0;
#pragma unroll
            for (int i = 0; i < 16; ++i) cp += (gb[i] >> g) & (pb[i] >> p) & 1u;
            if (cp) atomicAdd(&cntl[g * LM_BLOCK + p], cp);
        }
    }
    for (unsigned mp = ap; mp; mp &= mp - 1) {
        const int p = __ffs(mp) - 1;
        unsigned c = 0;
#pragma unroll
        for (int i = 0; i < 16; ++i) c += (pb[i] >> p) & 1u;
        if (c) atomicAdd(&cntl[LM_BLOCK * LM_BLOCK + LM_BLOCK + p], c);
    }
    __syncthreads();
    const long tab = T.cnt_off[img];
    for (int i = tid; i < LM_BLOCK * LM_BLOCK + 2 * LM_BLOCK; i += 256) {
        const unsigned c = cntl[i];
        if (!c) continue;
        long idx;
        if (i < LM_BLOCK * LM_BLOCK) idx = tab + (long)(g0 + i / LM_BLOCK) * P + (p0 + i % LM_BLOCK);
        else if (i < LM_BLOCK * LM_BLOCK + LM_BLOCK) {                   // a lane's own area: counted by the first block of its row / column
            if (p0 != 0) continue;
            idx = tab + (long)G * P + g0 + (i - LM_BLOCK * LM_BLOCK);
        } else {
            if (g0 != 0) continue;
            idx = tab + (long)G * P + G + p0 + (i - LM_BLOCK * LM_BLOCK - LM_BLOCK);
        }
        if (tab >= 0 && idx < n_tables) atomicAdd(counts + idx, (unsigned long long)c);
    }
}

static inline long lm_align16(long v) { return (v + 15) & ~15l; }

/* Bytes of hn_lane_metric_batch's workspace: spline coefficients and sweep scratch (14 float64 per point), the sample offsets and the lane
 * of every point, 16 bytes per sample.  -1 for an argument out of range. */
extern "C" long hn_lane_metric_ws_bytes(int n_lanes, long n_points, long sample_cap) {
    if (n_lanes < 0 || n_points < 0 || sample_cap < 0 || n_points > (1l << 28) || sample_cap > (1l << 28)) return -1;
    return 14 * 8 * n_points + lm_align16(4 * (n_points + 1)) + lm_align16(4 * n_points) + 16 * sample_cap + 16;
}

/* pts: DEVICE fp64 [n_points][2] = x, y of every lane's points, lanes back to back.  tab: DEVICE int32, back to back: lane_off
 * [n_lanes + 1], img_lane [N + 1], img_g [N], img_h [N], img_w [N], cnt_off [N], work [n_work][4] (struct LaneTabs above).  n_tiles = the
 * tiles of all work items (64 x 64 pixels; the grid).  sample_cap: samples the workspace holds.  counts: uint64 [n_counts], zeroed here:
 * [0, n_counts - 1) = the images' tables at their cnt_off (|g & p| [G][P], then |g| [G], |p| [P]), counts[n_counts - 1] = status word
 * (0; non-zero: a segment longer than 1e9 or more samples than sample_cap -- the tables are then incomplete).  Five stream operations. */
extern "C" int hn_lane_metric_batch(const double* pts, const int* tab, int N, int n_lanes, long n_points, int n_work, long n_tiles,
                                    long sample_cap, int lane_width, void* ws, long ws_bytes, void* counts, long n_counts, hipStream_t st) {
    HN_CHECK_ARG(tab && counts && N > 0 && n_lanes >= 0 && n_points >= 0 && n_work >= 0 && n_tiles >= 0 && n_counts >= 1 && lane_width > 0 &&
                 lane_width <= 16384 && n_tiles <= 0x7fffffffl && sample_cap >= 0);
    const long need = hn_lane_metric_ws_bytes(n_lanes, n_points, sample_cap);
    HN_CHECK_ARG(need >= 0);
    if (hipMemsetAsync(counts, 0, (size_t)n_counts * 8, st) != hipSuccess) return HN_ERR_LAUNCH;
    if (n_lanes == 0 || n_points == 0 || n_work == 0 || n_tiles == 0) return HN_OK;
    HN_CHECK_ARG(pts && ws && ws_bytes >= need && ((uintptr_t)ws & 15) == 0);
    char* w = (char*)ws;
    double* coef = (double*)w;                 w += 9 * 8 * n_points;
    double* scr = (double*)w;                  w += 5 * 8 * n_points;
    unsigned* off = (unsigned*)w;              w += lm_align16(4 * (n_points + 1));
    int* pt_lane = (int*)w;                    w += lm_align16(4 * n_points);
    int4* smp = (int4*)w;
    unsigned long long* status = (unsigned long long*)counts + (n_counts - 1);
    LaneTabs T;
    T.lane_off = tab;
    T.img_lane = T.lane_off + n_lanes + 1;
    T.img_g = T.img_lane + N + 1;
    T.img_h = T.img_g + N;
    T.img_w = T.img_h + N;
    T.cnt_off = T.img_w + N;
    T.work = T.cnt_off + N;
    if (hipMemsetAsync(off, 0, (size_t)(lm_align16(4 * (n_points + 1)) + lm_align16(4 * n_points)), st) != hipSuccess) return HN_ERR_LAUNCH;
    hipLaunchKernelGGL(lane_spline_kernel, dim3((unsigned)cdiv(n_lanes, 64)), dim3(64), 0, st, pts, T.lane_off, n_lanes, n_points, coef, scr, off,
                       pt_lane, status);
    hipLaunchKernelGGL(lane_scan_kernel, dim3(1), dim3(1024), 0, st, off, n_points, sample_cap, status);
    if (sample_cap > 0)
        hipLaunchKernelGGL(lane_sample_kernel, dim3((unsigned)cdiv(sample_cap, 256)), dim3(256), 0, st, pts, T.lane_off, n_lanes, n_points, coef, off,
                           pt_lane, sample_cap, smp);
    hipLaunchKernelGGL(lane_tile_kernel, dim3((unsigned)n_tiles), dim3(256), 0, st, smp, off, T, N, n_lanes, n_points, n_work, n_tiles, sample_cap,
                       2 * lane_width, (unsigned long long*)counts, n_counts - 1);
    HN_LAUNCH_CHECK();
}
