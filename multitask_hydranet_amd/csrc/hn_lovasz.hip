// Lovasz-softmax segmentation loss (segment.use_lovasz; head_seg/loss_lovasz.py lovasz_softmax with classes='present', per_image=False,
// ignore=255, called on softmax(seg logits) by model.py cal_loss) on device, no host synchronisation.
//
//   p = softmax(logits) per pixel (fp32).  Pixels are flattened in (n, h, w) order; label == ignore_index drops a pixel; a label outside
//   [0, C) that is not ignored is background for every class.  For each class c with at least one fg pixel ("present"):
//     e_i = |fg_i - p_c(i)| sorted DESCENDING; F_j / B_j = fg / bg count up to and including sorted position j, G = fg count;
//     J_j = 1 - (G - F_j) / (G + B_j);  loss_c = sum_j e_(j) (J_j - J_{j-1}),  J_{-1} = 0.
//   loss = mean of loss_c over the present classes (0, with a zero gradient, when no class is present).
//   Gradient (the J differences are constants, as in the reference): dloss/dp_c(i) = -sign(fg - p) (J_r - J_{r-1}) / n_present at i's rank r,
//   then through the softmax Jacobian.
//
// Ties: the order is error descending, then flattened pixel index ascending (torch.sort(stable=True, descending=True)).  The reference
// sorts unstably, so its per-pixel gradient inside a run of equal errors is unspecified; the loss is the same for any order inside a run
// (the run's weights telescope to J_end - J_start-1).  Ours is deterministic: the sort is a stable LSD radix sort.
//
// Pipeline (all classes at once; key / payload arrays are [C][P], ping-pong A <-> B):
//   1. key pass: key = bits(d), d = 1 - e in [0, 1] (ascending key = descending e, 30 bits), formed as p_c for a fg pixel and as the other
//      classes' softmax share for a bg pixel (no cancellation: the top of the order keeps fp32's relative precision); ignored pixels
//      0x3FFFFFFF (sort last);
//      payload = pixel index | fg << 31; per-class fg counts and the valid count (device side, integer atomics); the pass-0 digit
//      histogram of every tile.
//   2. three LSD passes of 10 bits: per-tile digit histogram [C][1024][tiles], a row scan of it (reduce-then-scan: no waiting between
//      workgroups inside a launch), a stable scatter (ranks inside a wave from ballots, across the four waves through LDS).
//   3. post-sort: per-tile fg counts, then per tile the exclusive fg / bg prefix along the sorted order, the weight J_j - J_{j-1}
//      (closed forms), the loss partial of the tile (fp32, fixed-order reduction) and g[i][c] = -sign(fg - p) * weight scattered back to
//      pixel order as fp32 [P][C] (aliasing the key buffer A, free after the sort).
//   4. finalize: loss = sum_c (sum of the class's tile partials, double, fixed order) / n_present.
//   Backward: dlogits = gout / n_present * p (g - <p, g>), the softmax recomputed; fp32 rows or the space-to-depth bf16 operand of the
//   phase-form output conv (the layout of hn_seg_loss_bwd_s2d).
// Every sum is integer or a fixed-order float reduction: results are bitwise reproducible.
#include "hn_common.h"

#define HN_SEG_MAXC 16
#define LV_THREADS 256
#define LV_ROUNDS 32
#define LV_TILE (LV_THREADS * LV_ROUNDS)
#define LV_BITS 10
#define LV_BINS 1024
#define LV_IGNORED 0x3FFFFFFFu

__device__ __forceinline__ unsigned long long lv_lanes_below() { return (1ull << __lane_id()) - 1ull; }

// lanes of the wave holding the same 10-bit digit (call with every lane of the wave; only meaningful for active lanes)
__device__ __forceinline__ unsigned long long lv_peers(unsigned d, bool active) {
    unsigned long long m = __ballot(active);
#pragma unroll
    for (int k = 0; k < LV_BITS; ++k) {
        const bool b = (d >> k) & 1u;
        const unsigned long long v = __ballot(b);
        m &= b ? v : ~v;
    }
    return m;
}

// exclusive scan of one value per thread over a 256-thread block; `total` = the block's sum.  sh: 4 words of LDS.
__device__ __forceinline__ unsigned lv_block_scan(unsigned v, unsigned* sh, unsigned& total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    unsigned x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned t = __shfl_up(x, o);
        if (lane >= o) x += t;
    }
    if (lane == 63) sh[w] = x;
    __syncthreads();
    unsigned pre = 0;
    total = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const unsigned t = sh[k];
        if (k < w) pre += t;
        total += t;
    }
    __syncthreads();
    return pre + x - v;
}

__device__ __forceinline__ long lv_label(const void* target, int tf, long m) {
    return tf ? (long)reinterpret_cast<const float*>(target)[m] : reinterpret_cast<const long*>(target)[m];
}

__global__ void lv_zero_kernel(unsigned* p, int n) {
    if ((int)threadIdx.x < n) p[threadIdx.x] = 0u;
}

// 1. key pass: one tile of LV_TILE pixels per workgroup, every class.  Dynamic LDS: C * 1024 histogram words + 32 count words.
template <int CT>
__global__ __launch_bounds__(LV_THREADS) void lv_key_kernel(const float* __restrict__ logits, int ldl, int Cr, const void* __restrict__ target,
                                                            int tf, int ignore_index, long P, long nblk, unsigned* __restrict__ keys,
                                                            unsigned* __restrict__ vals, unsigned* __restrict__ hist,
                                                            unsigned* __restrict__ counts, const unsigned char* __restrict__ vmask,
                                                            long HW) {
    extern __shared__ unsigned lv_sh[];
    const int C = CT > 0 ? CT : Cr;
    unsigned* sh = lv_sh;
    unsigned* shc = lv_sh + C * LV_BINS;
    for (int i = threadIdx.x; i < C * LV_BINS + 32; i += LV_THREADS) lv_sh[i] = 0u;
    __syncthreads();
    const long b = xcd_remap(blockIdx.x, gridDim.x);
    const unsigned long long lt = lv_lanes_below();
    const bool lane0 = __lane_id() == 0;
    for (int r = 0; r < LV_ROUNDS; ++r) {
        const long i = b * LV_TILE + r * LV_THREADS + threadIdx.x;
        const bool act = i < P;
        long y = ignore_index;
        float mx = 0.f, inv = 0.f;
        const float* row = logits + (act ? i : 0) * (long)ldl;
        if (act) {
            y = lv_label(target, tf, i);
            if (vmask && !vmask[i / HW]) y = ignore_index;             // a pixel of an unlabelled image (task mask): dropped like an ignored one
            mx = row[0];
            for (int c = 1; c < C; ++c) mx = fmaxf(mx, row[c]);
            float se = 0.f;
            for (int c = 0; c < C; ++c) se += expf(row[c] - mx);
            inv = 1.f / se;
        }
        const bool valid = act && y != ignore_index;
        const unsigned long long vb = __ballot(valid);
        if (lane0 && vb) atomicAdd(&shc[C], (unsigned)__popcll(vb));
        for (int c = 0; c < C; ++c) {
            const bool fg = valid && y == c;
            const unsigned long long fb = __ballot(fg);
            if (lane0 && fb) atomicAdd(&shc[c], (unsigned)__popcll(fb));
            unsigned key = LV_IGNORED;
            if (valid) {
                // key on d = 1 - e, formed without cancellation (fg: p_c; bg: the other classes' share), so that the order near the top
                // (e close to 1, where the weights are largest) keeps fp32's relative precision
                float q = 0.f;
                if (fg)
                    q = expf(row[c] - mx);
                else
                    for (int k = 0; k < C; ++k)
                        if (k != c) q += expf(row[k] - mx);
                key = __float_as_uint(fminf(q * inv, 1.f));
            }
            if (act) {
                keys[c * P + i] = key;
                vals[c * P + i] = (unsigned)i | (fg ? 0x80000000u : 0u);
            }
            const unsigned d = key & (LV_BINS - 1);
            const unsigned long long pm = lv_peers(d, act);
            if (act && (pm & lt) == 0) atomicAdd(&sh[c * LV_BINS + d], (unsigned)__popcll(pm));
        }
    }
    __syncthreads();
    for (int k = threadIdx.x; k < C * LV_BINS; k += LV_THREADS) hist[(long)k * nblk + b] = sh[k];
    if ((int)threadIdx.x <= C && shc[threadIdx.x]) atomicAdd(&counts[threadIdx.x], shc[threadIdx.x]);
}

// 2a. digit histogram of one tile of one class (passes 1, 2)
__global__ __launch_bounds__(LV_THREADS) void lv_hist_kernel(const unsigned* __restrict__ keys, long P, long nblk, int shift,
                                                             unsigned* __restrict__ hist) {
    __shared__ unsigned sh[LV_BINS];
    for (int k = threadIdx.x; k < LV_BINS; k += LV_THREADS) sh[k] = 0u;
    __syncthreads();
    const long lin = xcd_remap(blockIdx.x, gridDim.x);
    const long c = lin / nblk, b = lin - c * nblk;
    const unsigned* kc = keys + c * P;
    const unsigned long long lt = lv_lanes_below();
    for (int r = 0; r < LV_ROUNDS; ++r) {
        const long i = b * LV_TILE + r * LV_THREADS + threadIdx.x;
        const bool act = i < P;
        const unsigned d = act ? (kc[i] >> shift) & (LV_BINS - 1) : 0u;
        const unsigned long long pm = lv_peers(d, act);
        if (act && (pm & lt) == 0) atomicAdd(&sh[d], (unsigned)__popcll(pm));
    }
    __syncthreads();
    for (int k = threadIdx.x; k < LV_BINS; k += LV_THREADS) hist[(c * LV_BINS + k) * nblk + b] = sh[k];
}

// 2b. one (class, digit) row of the histogram: exclusive scan over the tiles in place, row total -> totals[class][digit]
__global__ __launch_bounds__(LV_THREADS) void lv_scan_kernel(unsigned* __restrict__ hist, long nblk, unsigned* __restrict__ totals) {
    __shared__ unsigned sh[4];
    unsigned* row = hist + (long)blockIdx.x * nblk;
    unsigned carry = 0;
    for (long base = 0; base < nblk; base += 4 * LV_THREADS) {
        const long j = base + 4 * threadIdx.x;
        unsigned v[4], s = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            v[k] = j + k < nblk ? row[j + k] : 0u;
            s += v[k];
        }
        unsigned tot;
        unsigned run = carry + lv_block_scan(s, sh, tot);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (j + k < nblk) row[j + k] = run;
            run += v[k];
        }
        carry += tot;
    }
    if (threadIdx.x == 0) totals[blockIdx.x] = carry;
}

// 2c. stable scatter of one tile of one class.  Items go round by round (256 consecutive items per round, thread order inside a round),
// so position in the tile = original order.  Inside a wave the rank among equal digits comes from the peer mask; the counts of the
// lower waves of the round come through wc[4][1024]; base[d] carries the running output position of digit d.
__global__ __launch_bounds__(LV_THREADS) void lv_scatter_kernel(const unsigned* __restrict__ kin, const unsigned* __restrict__ vin,
                                                                unsigned* __restrict__ kout, unsigned* __restrict__ vout, long P, long nblk,
                                                                int shift, const unsigned* __restrict__ hist,
                                                                const unsigned* __restrict__ totals) {
    __shared__ unsigned base[LV_BINS];
    __shared__ unsigned wc[4][LV_BINS];
    __shared__ unsigned sh[4];
    const long lin = xcd_remap(blockIdx.x, gridDim.x);
    const long c = lin / nblk, b = lin - c * nblk;
    {
        unsigned t[4], s = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            t[k] = totals[c * LV_BINS + 4 * threadIdx.x + k];
            s += t[k];
        }
        unsigned tot;
        unsigned run = lv_block_scan(s, sh, tot);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const long d = 4 * threadIdx.x + k;
            base[d] = run + hist[(c * LV_BINS + d) * nblk + b];
            run += t[k];
        }
    }
    for (int k = threadIdx.x; k < 4 * LV_BINS; k += LV_THREADS) (&wc[0][0])[k] = 0u;
    __syncthreads();
    const int w = threadIdx.x >> 6;
    const unsigned long long lt = lv_lanes_below();
    const unsigned* kc = kin + c * P;
    const unsigned* vc = vin + c * P;
    for (int r = 0; r < LV_ROUNDS; ++r) {
        const long i = b * LV_TILE + r * LV_THREADS + threadIdx.x;
        const bool act = i < P;
        const unsigned key = act ? kc[i] : 0u, val = act ? vc[i] : 0u;
        const unsigned d = (key >> shift) & (LV_BINS - 1);
        const unsigned long long pm = lv_peers(d, act);
        const bool leader = act && (pm & lt) == 0;
        const unsigned cnt = (unsigned)__popcll(pm);
        if (leader) wc[w][d] = cnt;
        __syncthreads();
        if (act) {
            unsigned pos = base[d] + (unsigned)__popcll(pm & lt);
            for (int k = 0; k < w; ++k) pos += wc[k][d];
            kout[c * P + pos] = key;
            vout[c * P + pos] = val;
        }
        __syncthreads();
        if (leader) {
            atomicAdd(&base[d], cnt);
            wc[w][d] = 0u;
        }
    }
}

// 3a. fg count of every sorted tile of every present class
__global__ __launch_bounds__(LV_THREADS) void lv_fgcount_kernel(const unsigned* __restrict__ vals, long P, long nblk, int C,
                                                                const unsigned* __restrict__ counts, unsigned* __restrict__ blkfg) {
    __shared__ unsigned sh[4];
    const long lin = xcd_remap(blockIdx.x, gridDim.x);
    const long c = lin / nblk, b = lin - c * nblk;
    const long V = counts[C];
    unsigned s = 0;
    if (counts[c] > 0)
        for (int r = 0; r < LV_ROUNDS; ++r) {
            const long j = b * LV_TILE + r * LV_THREADS + threadIdx.x;
            if (j < V) s += vals[c * P + j] >> 31;
        }
    unsigned tot;
    lv_block_scan(s, sh, tot);
    if (threadIdx.x == 0) blkfg[c * nblk + b] = tot;
}

// 3b. weights, loss partials and the per-pixel gradient of one sorted tile
__global__ __launch_bounds__(LV_THREADS) void lv_post_kernel(const unsigned* __restrict__ keys, const unsigned* __restrict__ vals, long P,
                                                             long nblk, int C, const unsigned* __restrict__ counts,
                                                             const unsigned* __restrict__ blkfg, float* __restrict__ g,
                                                             float* __restrict__ part) {
    __shared__ unsigned sh[4];
    __shared__ float red[4];
    const long lin = xcd_remap(blockIdx.x, gridDim.x);
    const long c = lin / nblk, b = lin - c * nblk;
    const unsigned G = counts[c];
    const long V = counts[C];
    if (G == 0 || b * LV_TILE >= V) {
        if (threadIdx.x == 0) part[c * nblk + b] = 0.f;
        return;
    }
    unsigned s = 0;
    for (long k = threadIdx.x; k < b; k += LV_THREADS) s += blkfg[c * nblk + k];
    unsigned carry;
    lv_block_scan(s, sh, carry);                      // fg pixels in front of this tile
    const unsigned long long lt = lv_lanes_below();
    const int w = threadIdx.x >> 6;
    const float Gf = (float)G;
    float acc = 0.f;
    for (int r = 0; r < LV_ROUNDS; ++r) {
        const long j = b * LV_TILE + r * LV_THREADS + threadIdx.x;
        const bool act = j < V;
        const unsigned val = act ? vals[c * P + j] : 0u;
        const bool fg = act && (val >> 31);
        const unsigned long long fb = __ballot(fg);
        if (__lane_id() == 0) sh[w] = (unsigned)__popcll(fb);
        __syncthreads();
        unsigned pre = 0, tot = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const unsigned t = sh[k];
            if (k < w) pre += t;
            tot += t;
        }
        __syncthreads();
        if (act) {
            const unsigned F = carry + pre + (unsigned)__popcll(fb & lt);    // fg count before j
            const unsigned B = (unsigned)j - F;                               // bg count before j
            const float d = __uint_as_float(keys[c * P + j]);          // 1 - e
            const float e = 1.f - d;
            const float gb = Gf + (float)B;
            const float wt = fg ? 1.f / gb : (float)(G - F) / (gb * (gb + 1.f));
            acc += e * wt;
            g[(long)(val & 0x7FFFFFFFu) * C + c] = d < 1.f ? (fg ? -wt : wt) : 0.f;
        }
        carry += tot;
    }
    acc = wave_sum(acc);
    if (__lane_id() == 0) red[w] = acc;
    __syncthreads();
    if (threadIdx.x == 0) part[c * nblk + b] = (red[0] + red[1]) + (red[2] + red[3]);
}

// 4. loss = sum over present classes of the class's tile partials (double, fixed order) / n_present
__global__ __launch_bounds__(LV_THREADS) void lv_finalize_kernel(const float* __restrict__ part, long nblk, int C,
                                                                 const unsigned* __restrict__ counts, float* __restrict__ out) {
    __shared__ double red[4];
    double tot = 0.0;
    int np = 0;
    for (int c = 0; c < C; ++c) {
        if (counts[c] == 0) continue;
        ++np;
        double s = 0.0;
        for (long k = threadIdx.x; k < nblk; k += LV_THREADS) s += part[c * nblk + k];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
        __syncthreads();
        tot += (red[0] + red[1]) + (red[2] + red[3]);
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = np > 0 ? (float)(tot / np) : 0.f;
}

// ---- backward --------------------------------------------------------------------------------------------------------------------
// gradient of one pixel: st(c, value) for every class (zeros for an ignored pixel).  pmask: present classes; scale = gout / n_present.
template <int CT, typename Store>
__device__ __forceinline__ void lv_pixel_grad(const float* __restrict__ logits, int ldl, int C, const void* __restrict__ target, int tf,
                                              int ignore_index, long m, const float* __restrict__ g, unsigned pmask, float scale, Store st,
                                              const unsigned char* __restrict__ vmask, long HW) {
    const long y = lv_label(target, tf, m);
    if (y == ignore_index || scale == 0.f || (vmask && !vmask[m / HW])) {
        for (int c = 0; c < C; ++c) st(c, 0.f);
        return;
    }
    const float* row = logits + m * ldl;
    const float* gr = g + m * C;
    float mx = row[0];
    for (int c = 1; c < C; ++c) mx = fmaxf(mx, row[c]);
    float se = 0.f;
    for (int c = 0; c < C; ++c) se += expf(row[c] - mx);
    const float inv = 1.f / se;
    float dot = 0.f;
    for (int c = 0; c < C; ++c)
        if ((pmask >> c) & 1u) dot += expf(row[c] - mx) * inv * gr[c];
    for (int c = 0; c < C; ++c) {
        const float gc = ((pmask >> c) & 1u) ? gr[c] : 0.f;
        st(c, scale * (expf(row[c] - mx) * inv) * (gc - dot));
    }
}

__device__ __forceinline__ void lv_present(const unsigned* counts, int C, const float* gout, unsigned& pmask, float& scale) {
    pmask = 0u;
    int np = 0;
    for (int c = 0; c < C; ++c)
        if (counts[c] > 0) {
            pmask |= 1u << c;
            ++np;
        }
    scale = np > 0 ? gout[0] / (float)np : 0.f;
}

template <int CT>
__global__ __launch_bounds__(256) void lv_bwd_kernel(const float* __restrict__ logits, int ldl, int Cr, const void* __restrict__ target, int tf,
                                                     int ignore_index, long P, const float* __restrict__ g, const unsigned* __restrict__ counts,
                                                     const float* __restrict__ gout, float* __restrict__ dl, int ldd,
                                                     const unsigned char* __restrict__ vmask, long HW) {
    const int C = CT > 0 ? CT : Cr;
    unsigned pmask;
    float scale;
    lv_present(counts, C, gout, pmask, scale);
    for (long m = (long)blockIdx.x * 256 + threadIdx.x; m < P; m += (long)gridDim.x * 256) {
        float* d = dl + m * ldd;
        lv_pixel_grad<CT>(logits, ldl, C, target, tf, ignore_index, m, g, pmask, scale, [=](int c, float v) { d[c] = v; }, vmask, HW);
    }
}

// space-to-depth form: dz bf16 [N][H/2][W/2][ldz], channel (py*2+px)*C + c of low-res pixel (y, x) = dlogits(2y+py, 2x+px, c), zeros in
// [4C, ldz); one thread per low-res pixel writes its row
template <int CT>
__global__ __launch_bounds__(256) void lv_bwd_s2d_kernel(const float* __restrict__ logits, int ldl, int Cr, const void* __restrict__ target,
                                                         int tf, int ignore_index, int H, int W, long M4, const float* __restrict__ g,
                                                         const unsigned* __restrict__ counts, const float* __restrict__ gout,
                                                         bf16* __restrict__ dz, int ldz, const unsigned char* __restrict__ vmask) {
    const int C = CT > 0 ? CT : Cr;
    unsigned pmask;
    float scale;
    lv_present(counts, C, gout, pmask, scale);
    const int h = H >> 1, w = W >> 1;
    const long HW = (long)H * W;
    for (long q = (long)blockIdx.x * 256 + threadIdx.x; q < M4; q += (long)gridDim.x * 256) {
        const int x = (int)(q % w);
        const long t = q / w;
        const int y = (int)(t % h);
        const int n = (int)(t / h);
        bf16* d = dz + q * ldz;
#pragma unroll
        for (int ph = 0; ph < 4; ++ph) {
            const long m = (long)n * HW + (long)(2 * y + (ph >> 1)) * W + 2 * x + (ph & 1);
            bf16* dp = d + ph * C;
            lv_pixel_grad<CT>(logits, ldl, C, target, tf, ignore_index, m, g, pmask, scale, [=](int c, float v) { dp[c] = f2bf(v); }, vmask, HW);
        }
        for (int c = 4 * C; c < ldz; ++c) d[c] = f2bf(0.f);
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// workspace: keysA | valsA | keysB | valsB (u32 [C][P] each; g fp32 [P][C] aliases keysA after the sort) | hist u32 [C][1024][tiles] |
// totals u32 [C][1024] | counts u32 [32] (fg count per class, then the valid count at [C]) | blkfg u32 [C][tiles] | part fp32 [C][tiles]
struct LvWs {
    unsigned *keysA, *valsA, *keysB, *valsB, *hist, *totals, *counts, *blkfg;
    float* part;
    long nblk;
};

static inline long lv_align(long x) { return (x + 255) & ~255L; }

static long lv_layout(int N, long HW, int C, void* ws, LvWs* L) {
    const long P = (long)N * HW, nblk = (P + LV_TILE - 1) / LV_TILE;
    const long arr = lv_align((long)C * P * 4);
    long off[10];
    off[0] = 0;
    off[1] = off[0] + arr;
    off[2] = off[1] + arr;
    off[3] = off[2] + arr;
    off[4] = off[3] + arr;
    off[5] = off[4] + lv_align((long)C * LV_BINS * nblk * 4);
    off[6] = off[5] + lv_align((long)C * LV_BINS * 4);
    off[7] = off[6] + 256;
    off[8] = off[7] + lv_align((long)C * nblk * 4);
    off[9] = off[8] + lv_align((long)C * nblk * 4);
    if (L) {
        char* w = (char*)ws;
        L->keysA = (unsigned*)(w + off[0]);
        L->valsA = (unsigned*)(w + off[1]);
        L->keysB = (unsigned*)(w + off[2]);
        L->valsB = (unsigned*)(w + off[3]);
        L->hist = (unsigned*)(w + off[4]);
        L->totals = (unsigned*)(w + off[5]);
        L->counts = (unsigned*)(w + off[6]);
        L->blkfg = (unsigned*)(w + off[7]);
        L->part = (float*)(w + off[8]);
        L->nblk = nblk;
    }
    return off[9];
}

extern "C" long hn_seg_lovasz_ws_bytes(int N, long HW, int C) {
    if (N <= 0 || HW <= 0 || C < 2 || C > HN_SEG_MAXC) return 0;
    return lv_layout(N, HW, C, nullptr, nullptr);
}

static std::atomic<unsigned long long> g_lv_key_lds{0};

// (valid: the seg row of the task masks, uint8 [N]; nullptr = every image labelled.  Same launches either way.)
static int seg_lovasz_fwd(const float* logits, int ldl, int C, const void* target, int target_is_float, int ignore_index, int N,
                          long HW, void* ws, float* out, const unsigned char* valid, hipStream_t st) {
    HN_CHECK_ARG(logits && target && ws && out && C >= 2 && C <= HN_SEG_MAXC && ldl >= C && N > 0 && HW > 0);
    const long P = (long)N * HW;
    HN_CHECK_ARG(P <= 0x7FFFFFFFL);                  // pixel index + fg bit in one 32-bit payload
    LvWs L;
    lv_layout(N, HW, C, ws, &L);
    const long nblk = L.nblk;
    const size_t key_lds = ((size_t)C * LV_BINS + 32) * 4;
    if (key_lds > 64 * 1024) {
        if (!lds_optin(g_lv_key_lds, {(const void*)lv_key_kernel<0>})) return HN_ERR_LAUNCH;
    }
    hipLaunchKernelGGL(lv_zero_kernel, dim3(1), dim3(64), 0, st, L.counts, 32);
    if (C == 5)
        hipLaunchKernelGGL(lv_key_kernel<5>, dim3((unsigned)nblk), dim3(LV_THREADS), key_lds, st, logits, ldl, C, target, target_is_float,
                           ignore_index, P, nblk, L.keysA, L.valsA, L.hist, L.counts, valid, HW);
    else
        hipLaunchKernelGGL(lv_key_kernel<0>, dim3((unsigned)nblk), dim3(LV_THREADS), key_lds, st, logits, ldl, C, target, target_is_float,
                           ignore_index, P, nblk, L.keysA, L.valsA, L.hist, L.counts, valid, HW);
    const dim3 tiles((unsigned)(C * nblk)), rows((unsigned)(C * LV_BINS));
    unsigned *kin = L.keysA, *vin = L.valsA, *kout = L.keysB, *vout = L.valsB;
    for (int pass = 0; pass < 3; ++pass) {
        const int shift = pass * LV_BITS;
        if (pass > 0) hipLaunchKernelGGL(lv_hist_kernel, tiles, dim3(LV_THREADS), 0, st, kin, P, nblk, shift, L.hist);
        hipLaunchKernelGGL(lv_scan_kernel, rows, dim3(LV_THREADS), 0, st, L.hist, nblk, L.totals);
        hipLaunchKernelGGL(lv_scatter_kernel, tiles, dim3(LV_THREADS), 0, st, kin, vin, kout, vout, P, nblk, shift, L.hist, L.totals);
        unsigned* t = kin; kin = kout; kout = t;
        t = vin; vin = vout; vout = t;
    }
    // sorted: keysB / valsB (three passes); keysA is free and takes g
    hipLaunchKernelGGL(lv_fgcount_kernel, tiles, dim3(LV_THREADS), 0, st, L.valsB, P, nblk, C, L.counts, L.blkfg);
    hipLaunchKernelGGL(lv_post_kernel, tiles, dim3(LV_THREADS), 0, st, L.keysB, L.valsB, P, nblk, C, L.counts, L.blkfg, (float*)L.keysA, L.part);
    hipLaunchKernelGGL(lv_finalize_kernel, dim3(1), dim3(LV_THREADS), 0, st, L.part, nblk, C, L.counts, out);
    HN_LAUNCH_CHECK();
}
extern "C" int hn_seg_lovasz_fwd(const float* logits, int ldl, int C, const void* target, int target_is_float, int ignore_index, int N,
                                 long HW, void* ws, float* out, hipStream_t st) {
    return seg_lovasz_fwd(logits, ldl, C, target, target_is_float, ignore_index, N, HW, ws, out, nullptr, st);
}
extern "C" int hn_seg_lovasz_fwd_masked(const float* logits, int ldl, int C, const void* target, int target_is_float, int ignore_index, int N,
                                        long HW, const unsigned char* valid, void* ws, float* out, hipStream_t st) {
    HN_CHECK_ARG(valid);
    return seg_lovasz_fwd(logits, ldl, C, target, target_is_float, ignore_index, N, HW, ws, out, valid, st);
}

static int seg_lovasz_bwd(const float* logits, int ldl, int C, const void* target, int target_is_float, int ignore_index, int N,
                          long HW, const void* ws, const float* gout, float* dlogits, int ldd, const unsigned char* valid, hipStream_t st) {
    HN_CHECK_ARG(logits && target && ws && gout && dlogits && C >= 2 && C <= HN_SEG_MAXC && ldl >= C && ldd >= C && N > 0 && HW > 0);
    const long P = (long)N * HW;
    HN_CHECK_ARG(P <= 0x7FFFFFFFL);
    LvWs L;
    lv_layout(N, HW, C, const_cast<void*>(ws), &L);
    long blocks = (P + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    if (C == 5)
        hipLaunchKernelGGL(lv_bwd_kernel<5>, dim3((unsigned)blocks), dim3(256), 0, st, logits, ldl, C, target, target_is_float, ignore_index, P,
                           (const float*)L.keysA, L.counts, gout, dlogits, ldd, valid, HW);
    else
        hipLaunchKernelGGL(lv_bwd_kernel<0>, dim3((unsigned)blocks), dim3(256), 0, st, logits, ldl, C, target, target_is_float, ignore_index, P,
                           (const float*)L.keysA, L.counts, gout, dlogits, ldd, valid, HW);
    HN_LAUNCH_CHECK();
}

extern "C" int hn_seg_lovasz_bwd(const float* logits, int ldl, int C, const void* target, int target_is_float, int ignore_index, int N,
                                 long HW, const void* ws, const float* gout, float* dlogits, int ldd, hipStream_t st) {
    return seg_lovasz_bwd(logits, ldl, C, target, target_is_float, ignore_index, N, HW, ws, gout, dlogits, ldd, nullptr, st);
}
extern "C" int hn_seg_lovasz_bwd_masked(const float* logits, int ldl, int C, const void* target, int target_is_float, int ignore_index, int N,
                                        long HW, const unsigned char* valid, const void* ws, const float* gout, float* dlogits, int ldd,
                                        hipStream_t st) {
    HN_CHECK_ARG(valid);
    return seg_lovasz_bwd(logits, ldl, C, target, target_is_float, ignore_index, N, HW, ws, gout, dlogits, ldd, valid, st);
}

static int seg_lovasz_bwd_s2d(const float* logits, int ldl, int C, const void* target, int target_is_float, int ignore_index, int N,
                              int H, int W, const void* ws, const float* gout, void* dz, int ldz, const unsigned char* valid, hipStream_t st) {
    HN_CHECK_ARG(logits && target && ws && gout && dz && C >= 2 && C <= HN_SEG_MAXC && ldl >= C && N > 0 && H > 0 && W > 0 && !(H & 1) &&
                 !(W & 1) && ldz >= 4 * C);
    const long HW = (long)H * W, P = (long)N * HW;
    HN_CHECK_ARG(P <= 0x7FFFFFFFL);
    LvWs L;
    lv_layout(N, HW, C, const_cast<void*>(ws), &L);
    long blocks = (P / 4 + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    if (C == 5)
        hipLaunchKernelGGL(lv_bwd_s2d_kernel<5>, dim3((unsigned)blocks), dim3(256), 0, st, logits, ldl, C, target, target_is_float, ignore_index,
                           H, W, P / 4, (const float*)L.keysA, L.counts, gout, (bf16*)dz, ldz, valid);
    else
        hipLaunchKernelGGL(lv_bwd_s2d_kernel<0>, dim3((unsigned)blocks), dim3(256), 0, st, logits, ldl, C, target, target_is_float, ignore_index,
                           H, W, P / 4, (const float*)L.keysA, L.counts, gout, (bf16*)dz, ldz, valid);
    HN_LAUNCH_CHECK();
}
extern "C" int hn_seg_lovasz_bwd_s2d(const float* logits, int ldl, int C, const void* target, int target_is_float, int ignore_index, int N,
                                     int H, int W, const void* ws, const float* gout, void* dz, int ldz, hipStream_t st) {
    return seg_lovasz_bwd_s2d(logits, ldl, C, target, target_is_float, ignore_index, N, H, W, ws, gout, dz, ldz, nullptr, st);
}
extern "C" int hn_seg_lovasz_bwd_s2d_masked(const float* logits, int ldl, int C, const void* target, int target_is_float, int ignore_index,
                                            int N, int H, int W, const unsigned char* valid, const void* ws, const float* gout, void* dz, int ldz,
                                            hipStream_t st) {
    HN_CHECK_ARG(valid);
    return seg_lovasz_bwd_s2d(logits, ldl, C, target, target_is_float, ignore_index, N, H, W, ws, gout, dz, ldz, valid, st);
}
