// Lane filter by the seg head's marking class (deploy/src/model/hydranet_model.cpp:546-607; lane_codec.LaneSegFilter): after the
// lane NMS the survivors are capped at top_k, every one of them is painted as a thick polyline, and it is kept when more than min_ratio of
// its painted pixels lie on the arg-max map's lane_class.  The inputs are hn_lane_decode_nms's device outputs as they are; nothing crosses
// the host and no full-frame mask is written.
//   lane_select_kernel   one workgroup per image: the first top_k entries of `order` with keep != 0 (wave ballots keep the order), their
//                        points rounded to integers (ties to even, clamped to +-16383: draw.py's limit) into the workspace with the
//                        reach-inflated bounding box; stats and keep_out are defined here (rows zeroed, keep_out cleared)
//   lane_paint_kernel    one workgroup per 64 x 64 tile of one image: the tile of the int64 map becomes one class bit per pixel in LDS,
//                        once, and only when a selected lane's box meets the tile; every such lane is painted into a bit plane per wave
//                        (one wave per segment, a row of the tile per ballot: no atomics inside the tile) with draw_kernel's integer
//                        distance test (kind 0, hn_draw.hip), the union of the planes and its AND with the class plane are pop-counted,
//                        and both counts go into `stats` with integer atomics (exact, order independent)
//   lane_decide_kernel   one thread per selected lane: kept = (float)inter / (float)area > min_ratio (one fp32 division, strict: 0 / 0 is
//                        a NaN and drops the lane), and the survivors' keep_out entries are set
// No workgroup waits on another; three launches, no memset, no allocation, no synchronisation.
#include "hn_common.h"

#define LF_TILE 64
#define LF_MAX_TOPK 64
#define LF_MAX_PPL 1024
#define LF_LIM 16383                     // hn_draw's coordinate limit: the distance test's 64-bit products hold up to it
#define LF_META 8                        // ints per selected lane: anchor, position in order, start, end, box x0, x1, y0, y1

__device__ __forceinline__ int lf_reach(int t) { return (2 * t + 3) / 4 + 1; }       // draw_reach (hn_draw.hip): >= t / 2, rounded up, + 1

struct LaneFilterGeo {
    int N, W, H, hw, ppl, interval, top_k, line_width, lane_class;
    float min_ratio;
};

// meta: int32 [N][top_k][LF_META]; pts: int32 [N][top_k][ppl] = rounded x of position p (valid for start <= p < end)
__global__ __launch_bounds__(256) void lane_select_kernel(const float* __restrict__ X, const int* __restrict__ start, const int* __restrict__ end,
                                                          const int* __restrict__ order, const int* __restrict__ keep,
                                                          const int* __restrict__ counts, LaneFilterGeo g, int* __restrict__ meta,
                                                          int* __restrict__ pts, int* __restrict__ keep_out, int* __restrict__ stats,
                                                          int* __restrict__ n_sel) {
    __shared__ int s_j[LF_MAX_TOPK];
    __shared__ int s_n;
    const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const long row = (long)n * g.hw;
    for (int j = tid; j < g.hw; j += 256) keep_out[row + j] = 0;
    for (int i = tid; i < g.top_k * 4; i += 256) stats[(long)n * g.top_k * 4 + i] = 0;
    const int cnt = min(max(counts[n], 0), g.hw);
    if (tid < 64) {                                                      // wave 0: ordered compaction, 64 candidates at a time
        int found = 0;
        for (int base = 0; base < cnt && found < g.top_k; base += 64) {
            const int j = base + lane;
            const bool k = j < cnt && keep[row + j] != 0;
            const unsigned long long m = __ballot(k);
            const int pos = found + __popcll(m & ((1ull << lane) - 1ull));
            if (k && pos < g.top_k) s_j[pos] = j;
            found += __popcll(m);
        }
        if (lane == 0) s_n = min(found, g.top_k);
    }
    __syncthreads();
    const int ns = s_n;
    if (tid == 0) n_sel[n] = ns;
    if (tid >= ns) return;
    // one thread per selected lane: a handful of lanes of at most ppl points each
    const int k = tid, j = s_j[k];
    int a = order[row + j], s = 0, e = 0;
    const bool anchor_ok = a >= 0 && a < g.hw;
    if (anchor_ok) { s = start[row + a]; e = end[row + a]; }
    int* p_out = pts + ((long)n * g.top_k + k) * g.ppl;
    int bx0 = 1, bx1 = 0, by0 = 1, by1 = 0;                              // the empty box: a lane that paints nothing meets no tile
    if (anchor_ok && s >= 0 && e <= g.ppl && e - s >= 2) {
        const float* xr = X + (row + a) * g.ppl;
        int lo = LF_LIM, hi = -LF_LIM;
        bool finite = true;
        for (int p = s; p < e; ++p) {
            const float x = xr[p];
            if (!(fabsf(x) <= 3.0e38f)) { finite = false; break; }       // NaN or infinity: the lane paints nothing
            const int xi = min(max(__float2int_rn(x), -LF_LIM), LF_LIM); // cv::Point(Point2f): nearest, ties to even (saturating)
            p_out[p] = xi;
            lo = min(lo, xi);
            hi = max(hi, xi);
        }
        if (finite) {
            const int r = lf_reach(g.line_width);
            bx0 = lo - r; bx1 = hi + r;
            by0 = g.H - 1 - (e - 1) * g.interval - r;
            by1 = g.H - 1 - s * g.interval + r;
        }
    } else {
        s = e = 0;
    }
    if (bx0 > bx1) s = e = 0;
    int* m = meta + ((long)n * g.top_k + k) * LF_META;
    m[0] = a; m[1] = j; m[2] = s; m[3] = e; m[4] = bx0; m[5] = bx1; m[6] = by0; m[7] = by1;
    stats[((long)n * g.top_k + k) * 4] = j;
}

__global__ __launch_bounds__(256) void lane_paint_kernel(const long* __restrict__ mask, LaneFilterGeo g, const int* __restrict__ meta,
                                                         const int* __restrict__ pts, const int* __restrict__ n_sel, int* __restrict__ stats) {
    __shared__ unsigned long long s_cls[LF_TILE];                        // bit x of word y: pixel (X0 + x, Y0 + y) is of lane_class
    __shared__ unsigned long long s_pnt[4][LF_TILE];                     // what every wave painted of the current lane
    __shared__ int s_meta[LF_MAX_TOPK][LF_META];
    __shared__ int s_x[LF_MAX_PPL];
    const int n = blockIdx.z, tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int X0 = blockIdx.x * LF_TILE, Y0 = blockIdx.y * LF_TILE;
    if (X0 >= g.W || Y0 >= g.H) return;
    const int X1 = min(X0 + LF_TILE, g.W) - 1, Y1 = min(Y0 + LF_TILE, g.H) - 1;      // the tile's pixels, inside the image
    const int ns = min(max(n_sel[n], 0), g.top_k);
    for (int i = tid; i < ns * LF_META; i += 256) (&s_meta[0][0])[i] = meta[(long)n * g.top_k * LF_META + i];
    __syncthreads();
    bool any = false;
    for (int k = 0; k < ns; ++k)
        any = any || (s_meta[k][4] <= X1 && s_meta[k][5] >= X0 && s_meta[k][6] <= Y1 && s_meta[k][7] >= Y0);
    if (!any) return;                                                    // (uniform) no lane reaches this tile: its map is not read
    // the class plane: one row of the tile per wave and step, a ballot is the row's word; outside the image the bit is 0
    const long* mp = mask + (long)n * g.H * g.W;
    for (int y = wave; y < LF_TILE; y += 4) {
        const bool in = X0 + lane <= X1 && Y0 + y <= Y1;
        const bool c = in && mp[(long)(Y0 + y) * g.W + X0 + lane] == (long)g.lane_class;
        const unsigned long long m = __ballot(c);
        if (lane == 0) s_cls[y] = m;
    }
    const long r = lf_reach(g.line_width);
    const long t2 = (long)g.line_width * g.line_width;
    for (int k = 0; k < ns; ++k) {
        if (!(s_meta[k][4] <= X1 && s_meta[k][5] >= X0 && s_meta[k][6] <= Y1 && s_meta[k][7] >= Y0)) continue;      // uniform
        const int s = s_meta[k][2], e = s_meta[k][3];
        __syncthreads();                                                 // the previous lane's planes and points are counted
        const int* px = pts + ((long)n * g.top_k + k) * g.ppl;
        for (int p = s + tid; p < e; p += 256) s_x[p] = px[p];
        s_pnt[wave][lane] = 0;
        __syncthreads();
        for (int i = s + wave; i + 1 < e; i += 4) {                      // one wave per segment (p_i, p_{i+1})
            const long x0 = s_x[i], x1 = s_x[i + 1];
            const long y0 = g.H - 1 - (long)i * g.interval, y1 = y0 - g.interval;
            const int bx0 = (int)max(min(x0, x1) - r, (long)X0), bx1 = (int)min(max(x0, x1) + r, (long)X1);
            const int by0 = (int)max(min(y0, y1) - r, (long)Y0), by1 = (int)min(max(y0, y1) + r, (long)Y1);
            if (bx0 > bx1 || by0 > by1) continue;
            const long dx = x1 - x0, dy = y1 - y0, len2 = dx * dx + dy * dy;
            const int x = X0 + lane;
            const bool col = x >= bx0 && x <= bx1;
            for (int y = by0; y <= by1; ++y) {
                bool hit = false;
                if (col) {                                               // draw_covers, kind 0 (hn_draw.hip): 4 distance^2 <= thickness^2
                    const long qx = x - x0, qy = y - y0;
                    const long dot = qx * dx + qy * dy;
                    long num, den;
                    if (len2 == 0 || dot <= 0) { num = qx * qx + qy * qy; den = 1; }
                    else if (dot >= len2) { const long ex = x - x1, ey = y - y1; num = ex * ex + ey * ey; den = 1; }
                    else { const long cr = qx * dy - qy * dx; num = cr * cr; den = len2; }
                    hit = num <= ((t2 * den) >> 2);
                }
                const unsigned long long m = __ballot(hit);
                if (lane == 0 && m) s_pnt[wave][y - Y0] |= m;            // the wave's own plane: no other wave writes it
            }
        }
        __syncthreads();
        if (wave == 0) {
            const unsigned long long w = s_pnt[0][lane] | s_pnt[1][lane] | s_pnt[2][lane] | s_pnt[3][lane];
            int area = __popcll(w), inter = __popcll(w & s_cls[lane]);
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) {
                area += __shfl_xor(area, d, 64);
                inter += __shfl_xor(inter, d, 64);
            }
            if (lane == 0 && area) {
                int* st = stats + ((long)n * g.top_k + k) * 4;
                atomicAdd(st + 1, area);
                if (inter) atomicAdd(st + 2, inter);
            }
        }
    }
}

__global__ __launch_bounds__(64) void lane_decide_kernel(LaneFilterGeo g, const int* __restrict__ n_sel, int* __restrict__ stats,
                                                         int* __restrict__ keep_out) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= g.N * g.top_k) return;
    const int n = i / g.top_k, k = i - n * g.top_k;
    if (k >= min(max(n_sel[n], 0), g.top_k)) return;
    int* st = stats + (long)i * 4;
    const int j = st[0];
    const bool kept = __fdiv_rn((float)st[2], (float)st[1]) > g.min_ratio;          // 0 / 0: NaN, not greater
    st[3] = kept ? 1 : 0;
    if (kept && j >= 0 && j < g.hw) keep_out[(long)n * g.hw + j] = 1;
}

/* Bytes of hn_lane_seg_filter's workspace: 8 ints and ppl rounded x per selected lane.  -1 for an argument out of range
 * (N < 1, top_k outside 1 .. 64, ppl outside 1 .. 1024). */
extern "C" long hn_lane_seg_filter_ws_bytes(int N, int top_k, int ppl) {
    if (N < 1 || N > 65535 || top_k < 1 || top_k > LF_MAX_TOPK || ppl < 1 || ppl > LF_MAX_PPL) return -1;
    return (long)N * top_k * (LF_META + ppl) * 4;
}

extern "C" int hn_lane_seg_filter(const float* X, const int* start, const int* end, const int* order, const int* keep, const int* counts, int N,
                                  int W, int H, int stride, int ppl, int interval, const long* mask, int lane_class, int line_width,
                                  float min_ratio, int top_k, void* ws, long ws_bytes, int* keep_out, int* stats, int* n_sel, hipStream_t st) {
    HN_CHECK_ARG(X && start && end && order && keep && counts && mask && ws && keep_out && stats && n_sel);
    HN_CHECK_ARG(top_k >= 1 && top_k <= LF_MAX_TOPK && line_width >= 1 && line_width <= 16384 && stride > 0 && interval > 0);
    HN_CHECK_ARG(W > 0 && H > 0 && W <= 16384 && H <= 16384 && W % stride == 0 && H % stride == 0);
    const long need = hn_lane_seg_filter_ws_bytes(N, top_k, ppl);
    HN_CHECK_ARG(need >= 0 && ws_bytes >= need && ((uintptr_t)ws & 3) == 0);
    HN_CHECK_ARG((long)(ppl - 1) * interval <= (long)LF_LIM + H - 1);    // every y = H - 1 - p interval stays within the limit
    const long hw = (long)(W / stride) * (H / stride);
    HN_CHECK_ARG(hw <= 0x7fffffffl / ppl);
    LaneFilterGeo g;
    g.N = N; g.W = W; g.H = H; g.hw = (int)hw; g.ppl = ppl; g.interval = interval; g.top_k = top_k; g.line_width = line_width;
    g.lane_class = lane_class; g.min_ratio = min_ratio;
    int* meta = (int*)ws;
    int* pts = meta + (long)N * top_k * LF_META;
    hipLaunchKernelGGL(lane_select_kernel, dim3((unsigned)N), dim3(256), 0, st, X, start, end, order, keep, counts, g, meta, pts, keep_out, stats,
                       n_sel);
    hipLaunchKernelGGL(lane_paint_kernel, dim3((unsigned)cdiv(W, LF_TILE), (unsigned)cdiv(H, LF_TILE), (unsigned)N), dim3(256), 0, st, mask, g,
                       (const int*)meta, (const int*)pts, (const int*)n_sel, stats);
    hipLaunchKernelGGL(lane_decide_kernel, dim3((unsigned)cdiv((long)N * top_k, 64)), dim3(64), 0, st, g, (const int*)n_sel, stats, keep_out);
    HN_LAUNCH_CHECK();
}
