// Loss kernels of HydraNet.cal_loss (model/model.py:201-264) on device, no host synchronisation.
//   * segmentation: weighted cross entropy with ignore_index and "top-k hardest pixels" (head_seg/segmentation_loss.py:48-65).  The
//     reference sorts the 524,288 per-pixel losses of every image and averages the first k; the mean only needs the k-th largest value,
//     so a 3-level (11+11+10 bit) radix select on the fp32 bit pattern replaces the sort: exact, deterministic (integer atomics only).
//   * deploy-mode argmax over the class logits (model/model.py:197) -> int64 mask.
#include "hn_common.h"
#include "hn_det_common.h"      // the per-image task masks (hn_image_valid, hn_count_valid)

#define HN_SEG_MAXC 16

// per pixel: loss = w[y] * (logsumexp(l) - l[y]) (0 for ignored pixels); also the level-0 histogram (top 11 bits) per image
__global__ __launch_bounds__(256) void seg_ce_fwd_kernel(const float* logits, int ldl, int C, const void* target, int target_is_float,
                                                         const float* cw, int ignore_index, long HW, long M, float* loss,
                                                         unsigned int* hist /* [N][2048] or null */, const unsigned char* valid) {
    __shared__ unsigned int sh[2048];
    const bool do_hist = hist != nullptr;
    if (do_hist) {
        for (int i = threadIdx.x; i < 2048; i += 256) sh[i] = 0;
        __syncthreads();
    }
    // one block handles a contiguous pixel range inside ONE image (grid = N * blocks_per_image)
    const int bpi = gridDim.x / (int)(M / HW);
    const int n = blockIdx.x / bpi, b = blockIdx.x - n * bpi;
    const long per = (HW + bpi - 1) / bpi;
    const long p0 = (long)n * HW + b * per;
    long p1 = p0 + per;
    if (p1 > (long)(n + 1) * HW) p1 = (long)(n + 1) * HW;
    // an unlabelled image: every pixel as if ignored.  Its histograms stay empty at every level (its HW zero losses would all land in bin
    // 0, one LDS address): no bin stops the select's walk, which then ends at bin 0 with the whole rank left over, as it does for HW
    // zeros -- prefix 0, remaining k either way
    const bool lab = hn_image_valid(valid, n);
    for (long m = p0 + threadIdx.x; m < p1; m += 256) {
        const int y = target_is_float ? (int)reinterpret_cast<const float*>(target)[m] : (int)reinterpret_cast<const long*>(target)[m];
        float l = 0.f;
        if (lab && y != ignore_index && y >= 0 && y < C) {
            const float* row = logits + m * ldl;
            float mx = row[0];
            for (int c = 1; c < C; ++c) mx = fmaxf(mx, row[c]);
            float se = 0.f;
            for (int c = 0; c < C; ++c) se += __expf(row[c] - mx);
            l = cw[y] * (mx + __logf(se) - row[y]);
            if (l < 0.f) l = 0.f;                     // guards the unsigned-bit-pattern ordering (rounding can give -0)
        }
        loss[m] = l;
        if (do_hist && lab) atomicAdd(&sh[__float_as_uint(l) >> 21], 1u);
    }
    if (do_hist) {
        __syncthreads();
        for (int i = threadIdx.x; i < 2048; i += 256)
            if (sh[i]) atomicAdd(&hist[(long)n * 2048 + i], sh[i]);
    }
}

// compile-time class count, four consecutive pixels per thread: 4*CT contiguous floats = CT float4 loads, float4 targets, float4 loss store
template <int CT>
__global__ __launch_bounds__(256) void seg_ce_fwd_vec_kernel(const float* logits, const float* target, const float* cw, int ignore_index,
                                                             long HW, long M, float* loss, unsigned int* hist, const unsigned char* valid) {
    __shared__ unsigned int sh[2048];
    const bool do_hist = hist != nullptr;
    if (do_hist) {
        for (int i = threadIdx.x; i < 2048; i += 256) sh[i] = 0;
        __syncthreads();
    }
    const int bpi = gridDim.x / (int)(M / HW);
    const int n = blockIdx.x / bpi, b = blockIdx.x - n * bpi;
    const long per = ((HW / 4 + bpi - 1) / bpi) * 4;                  // pixels per block, a multiple of 4 (HW % 4 == 0)
    const long p0 = (long)n * HW + b * per;
    long p1 = p0 + per;
    if (p1 > (long)(n + 1) * HW) p1 = (long)(n + 1) * HW;
    const bool lab = hn_image_valid(valid, n);
    for (long m = p0 + 4 * threadIdx.x; m < p1; m += 1024) {
        if (!lab) {                                                    // an unlabelled image: four zero losses, nothing read, no histogram
            *reinterpret_cast<f32x4*>(loss + m) = f32x4{0.f, 0.f, 0.f, 0.f};
            continue;
        }
        float lg[4 * CT];
        const f32x4* row = reinterpret_cast<const f32x4*>(logits + m * CT);
#pragma unroll
        for (int k = 0; k < CT; ++k) { const f32x4 v = row[k]; lg[4 * k] = v[0]; lg[4 * k + 1] = v[1]; lg[4 * k + 2] = v[2]; lg[4 * k + 3] = v[3]; }
        const f32x4 tg = *reinterpret_cast<const f32x4*>(target + m);
        f32x4 lo;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int y = (int)tg[u];
            float l = 0.f;
            if (lab && y != ignore_index && y >= 0 && y < CT) {
                const float* r = &lg[u * CT];
                float mx = r[0];
#pragma unroll
                for (int c = 1; c < CT; ++c) mx = fmaxf(mx, r[c]);
                float se = 0.f, ry = 0.f;
#pragma unroll
                for (int c = 0; c < CT; ++c) { se += __expf(r[c] - mx); ry = c == y ? r[c] : ry; }
                l = cw[y] * (mx + __logf(se) - ry);
                if (l < 0.f) l = 0.f;
            }
            lo[u] = l;
            if (do_hist) atomicAdd(&sh[__float_as_uint(l) >> 21], 1u);
        }
        *reinterpret_cast<f32x4*>(loss + m) = lo;
    }
    if (do_hist) {
        __syncthreads();
        for (int i = threadIdx.x; i < 2048; i += 256)
            if (sh[i]) atomicAdd(&hist[(long)n * 2048 + i], sh[i]);
    }
}

// radix-select state per image: prefix (bits fixed so far), remaining rank r (how many of the still-ambiguous bin are needed)
struct SelState { unsigned int prefix; unsigned int remaining; };

// level L histogram of the elements whose higher bits equal the prefix.  level 1: bits 20..10 (11 bits), level 2: bits 9..0 (10 bits)
__global__ __launch_bounds__(256) void seg_hist_kernel(const float* loss, long HW, long M, const SelState* st, int level, unsigned int* hist,
                                                       const unsigned char* valid) {
    __shared__ unsigned int sh[2048];
    const int bpi = gridDim.x / (int)(M / HW);
    const int n = blockIdx.x / bpi, b = blockIdx.x - n * bpi;
    if (!hn_image_valid(valid, n)) return;                            // (the whole workgroup: see seg_ce_fwd_kernel)
    for (int i = threadIdx.x; i < 2048; i += 256) sh[i] = 0;
    __syncthreads();
    const long per = (HW + bpi - 1) / bpi;
    const long p0 = (long)n * HW + b * per;
    long p1 = p0 + per;
    if (p1 > (long)(n + 1) * HW) p1 = (long)(n + 1) * HW;
    const unsigned int prefix = st[n].prefix;
    for (long m = p0 + threadIdx.x; m < p1; m += 256) {
        const unsigned int u = __float_as_uint(loss[m]);
        if (level == 1) { if ((u >> 21) == (prefix >> 21)) atomicAdd(&sh[(u >> 10) & 2047], 1u); }
        else if ((u >> 10) == (prefix >> 10)) atomicAdd(&sh[u & 1023], 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 2048; i += 256)
        if (sh[i]) atomicAdd(&hist[(long)n * 2048 + i], sh[i]);
}

// one wave per image: find the bin (from the top) in which the remaining rank falls and fix that bin's bits.  The 2048 bins are staged in
// LDS, every lane sums its contiguous chunk, a wave suffix-scan locates the chunk and its lane walks at most 32 bins (a single thread
// walking 2048 dependent global loads took 60 us).  Semantics of the serial walk: b runs from the top bin down to 1 and stops at the first
// bin with h[b] >= need, otherwise need -= h[b]; b = 0 if no bin stops it.
__global__ __launch_bounds__(64) void seg_select_kernel(unsigned int* hist, SelState* st, int level, unsigned int k) {
    __shared__ unsigned int sh[2048];
    __shared__ int s_b;
    __shared__ unsigned int s_need;
    const int n = blockIdx.x, lane = threadIdx.x;
    unsigned int* h = hist + (long)n * 2048;
    const int bins = level == 2 ? 1024 : 2048;
    const int per = bins / 64;
    for (int i = lane; i < bins; i += 64) sh[i] = h[i];
    const unsigned int need0 = level == 0 ? k : st[n].remaining;
    if (lane == 0) { s_b = 0; s_need = 0; }
    __syncthreads();
    unsigned int local = 0;
    for (int j = 0; j < per; ++j) {
        const int b = lane * per + j;
        if (b >= 1) local += sh[b];                                   // bin 0 never stops the walk, it only receives what is left
    }
    // above = sum of the chunks of all higher lanes (inclusive suffix scan minus own)
    unsigned int suf = local;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned int v = __shfl_down(suf, o);
        if (lane + o < 64) suf += v;
    }
    const unsigned int above = suf - local;
    // the walk stops inside this lane's chunk iff above < need0 <= above + local  (cumulative count from the top reaches need0 here)
    const bool mine = above < need0 && need0 <= above + local;
    if (mine) {
        unsigned int need = need0 - above;
        int b = lane * per + per - 1;
        for (; b > lane * per && b > 0; --b) {
            if (sh[b] >= need) break;
            need -= sh[b];
        }
        // b is now either the stopping bin or the lowest bin of the chunk (which must stop the walk because the chunk total reaches need)
        s_b = b;
        s_need = need;
    }
    const unsigned long long any = __ballot(mine);
    if (!any && lane == 0) {                                          // fewer than need0 elements above bin 0: the walk ends at b = 0
        s_b = 0;
        s_need = need0 - suf;                                         // lane 0's inclusive suffix = everything in bins >= 1
    }
    __syncthreads();
    if (lane == 0) {
        const int shift = level == 0 ? 21 : (level == 1 ? 10 : 0);
        const unsigned int prefix = (level == 0 ? 0u : st[n].prefix) | ((unsigned int)s_b << shift);
        st[n].prefix = prefix;
        st[n].remaining = s_need;                      // elements of bin b (at this resolution) that still belong to the top-k
    }
    for (int i = lane; i < 2048; i += 64) h[i] = 0;                   // ready for the next level
}

// per image: sum of the losses strictly above the threshold (partial sums per block); the `remaining` ties at the threshold are added
// in the finalize kernel
__global__ __launch_bounds__(256) void seg_topk_sum_kernel(const float* loss, long HW, long M, const SelState* st, int use_topk, float* psum) {
    __shared__ float red[4];
    const int bpi = gridDim.x / (int)(M / HW);
    const int n = blockIdx.x / bpi, b = blockIdx.x - n * bpi;
    const long per = (HW + bpi - 1) / bpi;
    const long p0 = (long)n * HW + b * per;
    long p1 = p0 + per;
    if (p1 > (long)(n + 1) * HW) p1 = (long)(n + 1) * HW;
    const unsigned int thr = use_topk ? st[n].prefix : 0u;
    float s = 0.f;
    for (long m = p0 + threadIdx.x; m < p1; m += 256) {
        const float v = loss[m];
        if (!use_topk || __float_as_uint(v) > thr) s += v;
    }
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) psum[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

// 1 / (labelled images x per_image), rounded to fp32 once like the host's (float)(1.0 / denom) of the unmasked call; 0 without any
__device__ __forceinline__ float seg_masked_inv_denom(const unsigned char* valid, int N, double per_image) {
    const int nv = hn_count_valid(valid, N);
    return nv > 0 ? (float)(1.0 / ((double)nv * per_image)) : 0.f;
}

// out = ( sum_blocks psum + sum_n remaining_n * thr_n ) / denom;  with a mask denom = labelled images x per_image (out = 0 without any):
// an unlabelled image's losses are all zero, so its partial sums and its threshold term add +0
__global__ __launch_bounds__(256) void seg_loss_finalize_kernel(const float* psum, int nblocks, const SelState* st, int N, int use_topk,
                                                                double denom, float* out, const unsigned char* valid, double per_image) {
    __shared__ double red[4];
    double s = 0.0;
    for (int i = threadIdx.x; i < nblocks; i += 256) s += psum[i];
    if (use_topk)
        for (int n = threadIdx.x; n < N; n += 256) s += (double)st[n].remaining * (double)__uint_as_float(st[n].prefix);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        if (valid) {
            const int nv = hn_count_valid(valid, N);
            out[0] = nv > 0 ? (float)((red[0] + red[1] + red[2] + red[3]) / ((double)nv * per_image)) : 0.f;
        } else {
            out[0] = (float)((red[0] + red[1] + red[2] + red[3]) / denom);
        }
    }
}

// backward: dlogits[m][c] = gout/denom * sel(m) * w[y] * (softmax_c - [c == y]);  sel = 1 above the threshold, remaining/ties at it, 0 below
__global__ __launch_bounds__(256) void seg_ce_bwd_kernel(const float* logits, int ldl, int C, const void* target, int target_is_float,
                                                         const float* cw, int ignore_index, long HW, long M, const float* loss,
                                                         const SelState* st, const unsigned int* ties, int use_topk, const float* gout,
                                                         float inv_denom, float* dlogits, int ldd, const unsigned char* valid,
                                                         double per_image) {
    const float gs = gout[0] * (valid ? seg_masked_inv_denom(valid, (int)(M / HW), per_image) : inv_denom);
    for (long m = (long)blockIdx.x * 256 + threadIdx.x; m < M; m += (long)gridDim.x * 256) {
        const int n = (int)(m / HW);
        const int y = target_is_float ? (int)reinterpret_cast<const float*>(target)[m] : (int)reinterpret_cast<const long*>(target)[m];
        float sel = 0.f;
        if (hn_image_valid(valid, n) && y != ignore_index && y >= 0 && y < C) {
            sel = 1.f;
            if (use_topk) {
                const unsigned int u = __float_as_uint(loss[m]), thr = st[n].prefix;
                if (u < thr) sel = 0.f;
                else if (u == thr) sel = (float)st[n].remaining / (float)(ties[n] > 0 ? ties[n] : 1u);
            }
        }
        float* d = dlogits + m * ldd;
        if (sel == 0.f) {
            for (int c = 0; c < C; ++c) d[c] = 0.f;
            continue;
        }
        const float* row = logits + m * ldl;
        float mx = row[0];
        for (int c = 1; c < C; ++c) mx = fmaxf(mx, row[c]);
        float e[HN_SEG_MAXC], se = 0.f;
        for (int c = 0; c < C; ++c) { e[c] = __expf(row[c] - mx); se += e[c]; }
        const float k = gs * sel * cw[y] / se;
        for (int c = 0; c < C; ++c) d[c] = k * e[c] - (c == y ? gs * sel * cw[y] : 0.f);
    }
}

// the same gradient written straight into the operand the phase-form output conv's backward consumes (ops.SegOutUp): bf16
// [N][H/2][W/2][ldz], channel (py*2+px)*C + c of low-res pixel (y, x) = dlogits(2y+py, 2x+px, c), zeros in [4C, ldz).  One thread per
// low-res pixel writes one contiguous row; the fp32 dlogits tensor (168 MB at 16 x 512 x 1024 x 5) and the separate space-to-depth pass
// over it are never materialised.
__global__ __launch_bounds__(256) void seg_ce_bwd_s2d_kernel(const float* logits, int ldl, int C, const void* target, int target_is_float,
                                                             const float* cw, int ignore_index, int H, int W, long M4, const float* loss,
                                                             const SelState* st, const unsigned int* ties, int use_topk, const float* gout,
                                                             float inv_denom, bf16* dz, int ldz, const unsigned char* valid, double per_image) {
    const float gs = gout[0] * (valid ? seg_masked_inv_denom(valid, (int)(M4 / ((long)(H >> 1) * (W >> 1))), per_image) : inv_denom);
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
            const int yy = target_is_float ? (int)reinterpret_cast<const float*>(target)[m] : (int)reinterpret_cast<const long*>(target)[m];
            float sel = 0.f;
            if (hn_image_valid(valid, n) && yy != ignore_index && yy >= 0 && yy < C) {
                sel = 1.f;
                if (use_topk) {
                    const unsigned int u = __float_as_uint(loss[m]), thr = st[n].prefix;
                    if (u < thr) sel = 0.f;
                    else if (u == thr) sel = (float)st[n].remaining / (float)(ties[n] > 0 ? ties[n] : 1u);
                }
            }
            if (sel == 0.f) {
                for (int c = 0; c < C; ++c) d[ph * C + c] = f2bf(0.f);
                continue;
            }
            const float* row = logits + m * ldl;
            float mx = row[0];
            for (int c = 1; c < C; ++c) mx = fmaxf(mx, row[c]);
            float e[HN_SEG_MAXC], se = 0.f;
            for (int c = 0; c < C; ++c) { e[c] = __expf(row[c] - mx); se += e[c]; }
            const float k = gs * sel * cw[yy] / se;
            for (int c = 0; c < C; ++c) d[ph * C + c] = f2bf(k * e[c] - (c == yy ? gs * sel * cw[yy] : 0.f));
        }
        for (int c = 4 * C; c < ldz; ++c) d[c] = f2bf(0.f);
    }
}

// The same for a compile-time class count with vector memory operations: per image row of the quad the two pixels' logits are 2*CT
// contiguous floats (8-byte aligned: float2 loads), targets / losses float2, and the 4*CT (+ padding) bf16 results leave as 16-byte stores
// (the generic kernel issues 4*CT two-byte stores and 4*CT + 8 scalar loads per thread: 265 us for 2 M pixels).
template <int CT, int LDZ>
__global__ __launch_bounds__(256) void seg_ce_bwd_s2d_vec_kernel(const float* logits, const float* target, const float* cw, int ignore_index,
                                                                 int H, int W, long M4, const float* loss, const SelState* st,
                                                                 const unsigned int* ties, int use_topk, const float* gout, float inv_denom,
                                                                 bf16* dz, const unsigned char* valid, double per_image) {
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    const float gs = gout[0] * (valid ? seg_masked_inv_denom(valid, (int)(M4 / ((long)(H >> 1) * (W >> 1))), per_image) : inv_denom);
    const int h = H >> 1, w = W >> 1;
    const long HW = (long)H * W;
    for (long q = (long)blockIdx.x * 256 + threadIdx.x; q < M4; q += (long)gridDim.x * 256) {
        const int x = (int)(q % w);
        const long t = q / w;
        const int y = (int)(t % h);
        const int n = (int)(t / h);
        const unsigned int thr = use_topk ? st[n].prefix : 0u;
        const float share = use_topk ? (float)st[n].remaining / (float)(ties[n] > 0 ? ties[n] : 1u) : 1.f;
        float lg[2][2 * CT];
        f32x2 tg[2], ls[2];
#pragma unroll
        for (int py = 0; py < 2; ++py) {
            const long m = (long)n * HW + (long)(2 * y + py) * W + 2 * x;
            const f32x2* row = reinterpret_cast<const f32x2*>(logits + m * CT);
#pragma unroll
            for (int k = 0; k < CT; ++k) { const f32x2 v = row[k]; lg[py][2 * k] = v[0]; lg[py][2 * k + 1] = v[1]; }
            tg[py] = *reinterpret_cast<const f32x2*>(target + m);
            ls[py] = use_topk ? *reinterpret_cast<const f32x2*>(loss + m) : (f32x2){0.f, 0.f};
        }
        bf16 out[LDZ];
#pragma unroll
        for (int c = 0; c < LDZ; ++c) out[c] = f2bf(0.f);
#pragma unroll
        for (int ph = 0; ph < 4; ++ph) {
            const int py = ph >> 1, px = ph & 1;
            const int yy = (int)tg[py][px];
            float sel = 0.f;
            if (hn_image_valid(valid, n) && yy != ignore_index && yy >= 0 && yy < CT) {
                sel = 1.f;
                if (use_topk) {
                    const unsigned int u = __float_as_uint(ls[py][px]);
                    if (u < thr) sel = 0.f;
                    else if (u == thr) sel = share;
                }
            }
            if (sel != 0.f) {
                const float* r = &lg[py][px * CT];
                float mx = r[0];
#pragma unroll
                for (int c = 1; c < CT; ++c) mx = fmaxf(mx, r[c]);
                float e[CT], se = 0.f;
#pragma unroll
                for (int c = 0; c < CT; ++c) { e[c] = __expf(r[c] - mx); se += e[c]; }
                const float wy = cw[yy];
                const float k = gs * sel * wy / se;
#pragma unroll
                for (int c = 0; c < CT; ++c) out[ph * CT + c] = f2bf(k * e[c] - (c == yy ? gs * sel * wy : 0.f));
            }
        }
        bf16x8* d = reinterpret_cast<bf16x8*>(dz + q * LDZ);
#pragma unroll
        for (int k = 0; k < LDZ / 8; ++k) {
            bf16x8 v;
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = out[k * 8 + j];
            d[k] = v;
        }
    }
}

// number of elements exactly at the threshold, per image (for the tie share in backward): it is hist level-2 bin = prefix&1023, saved
// by the select kernel before clearing; simpler: count again
__global__ __launch_bounds__(256) void seg_count_ties_kernel(const float* loss, long HW, long M, const SelState* st, unsigned int* ties) {
    const int bpi = gridDim.x / (int)(M / HW);
    const int n = blockIdx.x / bpi, b = blockIdx.x - n * bpi;
    const long per = (HW + bpi - 1) / bpi;
    const long p0 = (long)n * HW + b * per;
    long p1 = p0 + per;
    if (p1 > (long)(n + 1) * HW) p1 = (long)(n + 1) * HW;
    const unsigned int thr = st[n].prefix;
    unsigned int c = 0;
    for (long m = p0 + threadIdx.x; m < p1; m += 256) c += __float_as_uint(loss[m]) == thr ? 1u : 0u;
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(&ties[n], c);
}

// deploy-mode argmax over C channel logits (NHWC fp32, first maximum wins like torch.argmax) -> int64
__global__ void argmax_kernel(const float* logits, int ldl, int C, long M, long* out) {
    for (long m = (long)blockIdx.x * blockDim.x + threadIdx.x; m < M; m += (long)gridDim.x * blockDim.x) {
        const float* row = logits + m * ldl;
        float best = row[0];
        int arg = 0;
        for (int c = 1; c < C; ++c)
            if (row[c] > best) { best = row[c]; arg = c; }
        out[m] = arg;
    }
}

// ---------------------------------------------------------------------------------------------------------
static inline int bpi_for(long HW) {
    long b = (HW + 4095) / 4096;
    if (b > 64) b = 64;
    return (int)(b < 1 ? 1 : b);
}

extern "C" int hn_seg_loss_blocks(int N, long HW) { return N * bpi_for(HW); }

// workspace layout (caller allocates, all zero-initialised by this call where needed):
//   loss fp32[M] | hist u32[N*2048] | state {u32,u32}[N] | ties u32[N] | psum fp32[blocks]
extern "C" long hn_seg_loss_ws_bytes(int N, long HW) {
    const long M = (long)N * HW;
    return M * 4 + (long)N * 2048 * 4 + (long)N * 8 + (long)N * 4 + (long)hn_seg_loss_blocks(N, HW) * 4 + 64;
}

__global__ void zero_u32_kernel(unsigned int* p, long n) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = 0u;
}

// forward: returns the scalar loss in out[0]; ws is kept for the backward pass.  k = int(top_k_ratio * HW) when use_topk.
// (valid: the seg row of the task masks, hn_det_common.h; nullptr = every image labelled.  Same launches either way.)
static int seg_loss_fwd(const float* logits, int ldl, int C, const void* target, int target_is_float, const float* cw,
                        int ignore_index, int N, long HW, int use_topk, long k, void* ws, float* out, const unsigned char* valid,
                        hipStream_t st) {
    HN_CHECK_ARG(logits && target && cw && ws && out && C >= 1 && C <= HN_SEG_MAXC && N > 0 && HW > 0 && (!use_topk || (k >= 1 && k <= HW)));
    const long M = (long)N * HW;
    char* w = (char*)ws;
    float* loss = (float*)w;
    unsigned int* hist = (unsigned int*)(w + M * 4);
    SelState* state = (SelState*)(w + M * 4 + (long)N * 2048 * 4);
    unsigned int* ties = (unsigned int*)(w + M * 4 + (long)N * 2048 * 4 + (long)N * 8);
    float* psum = (float*)(w + M * 4 + (long)N * 2048 * 4 + (long)N * 12);
    const int blocks = hn_seg_loss_blocks(N, HW);
    // zero the histogram + selection state with a kernel, not hipMemsetAsync: inside a captured hipGraph the memset node was observed to
    // lose its ordering against the following kernel (first replay after a host sync while another process shares the GPU -> NaN loss)
    {
        const long words = (long)N * 2048 + (long)N * 3;
        hipLaunchKernelGGL(zero_u32_kernel, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, st, hist, words);
    }
    if (C == 5 && ldl == 5 && target_is_float && (HW & 3) == 0 && (reinterpret_cast<uintptr_t>(logits) & 15) == 0 &&
        (reinterpret_cast<uintptr_t>(target) & 15) == 0)
        hipLaunchKernelGGL(seg_ce_fwd_vec_kernel<5>, dim3(blocks), dim3(256), 0, st, logits, (const float*)target, cw, ignore_index, HW, M, loss,
                           use_topk ? hist : (unsigned int*)nullptr, valid);
    else
        hipLaunchKernelGGL(seg_ce_fwd_kernel, dim3(blocks), dim3(256), 0, st, logits, ldl, C, target, target_is_float, cw, ignore_index, HW, M,
                           loss, use_topk ? hist : (unsigned int*)nullptr, valid);
    if (use_topk) {
        hipLaunchKernelGGL(seg_select_kernel, dim3(N), dim3(64), 0, st, hist, state, 0, (unsigned int)k);
        hipLaunchKernelGGL(seg_hist_kernel, dim3(blocks), dim3(256), 0, st, loss, HW, M, state, 1, hist, valid);
        hipLaunchKernelGGL(seg_select_kernel, dim3(N), dim3(64), 0, st, hist, state, 1, (unsigned int)k);
        hipLaunchKernelGGL(seg_hist_kernel, dim3(blocks), dim3(256), 0, st, loss, HW, M, state, 2, hist, valid);
        hipLaunchKernelGGL(seg_select_kernel, dim3(N), dim3(64), 0, st, hist, state, 2, (unsigned int)k);
        hipLaunchKernelGGL(seg_count_ties_kernel, dim3(blocks), dim3(256), 0, st, loss, HW, M, state, ties);
    }
    hipLaunchKernelGGL(seg_topk_sum_kernel, dim3(blocks), dim3(256), 0, st, loss, HW, M, state, use_topk, psum);
    const double denom = use_topk ? (double)N * (double)k : (double)M;
    hipLaunchKernelGGL(seg_loss_finalize_kernel, dim3(1), dim3(256), 0, st, psum, blocks, state, N, use_topk, denom, out, valid,
                       use_topk ? (double)k : (double)HW);
    HN_LAUNCH_CHECK();
}
extern "C" int hn_seg_loss_fwd(const float* logits, int ldl, int C, const void* target, int target_is_float, const float* cw,
                               int ignore_index, int N, long HW, int use_topk, long k, void* ws, float* out, hipStream_t st) {
    return seg_loss_fwd(logits, ldl, C, target, target_is_float, cw, ignore_index, N, HW, use_topk, k, ws, out, nullptr, st);
}
extern "C" int hn_seg_loss_fwd_masked(const float* logits, int ldl, int C, const void* target, int target_is_float, const float* cw,
                                      int ignore_index, int N, long HW, int use_topk, long k, const unsigned char* valid, void* ws, float* out,
                                      hipStream_t st) {
    HN_CHECK_ARG(valid);
    return seg_loss_fwd(logits, ldl, C, target, target_is_float, cw, ignore_index, N, HW, use_topk, k, ws, out, valid, st);
}

static int seg_loss_bwd(const float* logits, int ldl, int C, const void* target, int target_is_float, const float* cw,
                        int ignore_index, int N, long HW, int use_topk, long k, const void* ws, const float* gout, float* dlogits,
                        int ldd, const unsigned char* valid, hipStream_t st) {
    HN_CHECK_ARG(logits && target && cw && ws && gout && dlogits && C >= 1 && C <= HN_SEG_MAXC && N > 0 && HW > 0);
    const long M = (long)N * HW;
    const char* w = (const char*)ws;
    const float* loss = (const float*)w;
    const SelState* state = (const SelState*)(w + M * 4 + (long)N * 2048 * 4);
    const unsigned int* ties = (const unsigned int*)(w + M * 4 + (long)N * 2048 * 4 + (long)N * 8);
    const double denom = use_topk ? (double)N * (double)k : (double)M;
    long blocks = (M + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(seg_ce_bwd_kernel, dim3(blocks), dim3(256), 0, st, logits, ldl, C, target, target_is_float, cw, ignore_index, HW, M, loss,
                       state, ties, use_topk, gout, (float)(1.0 / denom), dlogits, ldd, valid, use_topk ? (double)k : (double)HW);
    HN_LAUNCH_CHECK();
}
extern "C" int hn_seg_loss_bwd(const float* logits, int ldl, int C, const void* target, int target_is_float, const float* cw,
                               int ignore_index, int N, long HW, int use_topk, long k, const void* ws, const float* gout, float* dlogits,
                               int ldd, hipStream_t st) {
    return seg_loss_bwd(logits, ldl, C, target, target_is_float, cw, ignore_index, N, HW, use_topk, k, ws, gout, dlogits, ldd, nullptr, st);
}
extern "C" int hn_seg_loss_bwd_masked(const float* logits, int ldl, int C, const void* target, int target_is_float, const float* cw,
                                      int ignore_index, int N, long HW, int use_topk, long k, const unsigned char* valid, const void* ws,
                                      const float* gout, float* dlogits, int ldd, hipStream_t st) {
    HN_CHECK_ARG(valid);
    return seg_loss_bwd(logits, ldl, C, target, target_is_float, cw, ignore_index, N, HW, use_topk, k, ws, gout, dlogits, ldd, valid, st);
}

/* hn_seg_loss_bwd writing the space-to-depth bf16 operand of the phase-form output conv's backward instead of fp32 dlogits:
 * dz [N][H/2][W/2][ldz], ldz >= 4*C (see seg_ce_bwd_s2d_kernel); H, W even */
static int seg_loss_bwd_s2d(const float* logits, int ldl, int C, const void* target, int target_is_float, const float* cw,
                            int ignore_index, int N, int H, int W, int use_topk, long k, const void* ws, const float* gout, void* dz,
                            int ldz, const unsigned char* valid, hipStream_t st) {
    HN_CHECK_ARG(logits && target && cw && ws && gout && dz && C >= 1 && C <= HN_SEG_MAXC && N > 0 && H > 0 && W > 0 && !(H & 1) && !(W & 1) &&
                 ldz >= 4 * C);
    const long HW = (long)H * W, M = (long)N * HW;
    const char* w = (const char*)ws;
    const float* loss = (const float*)w;
    const SelState* state = (const SelState*)(w + M * 4 + (long)N * 2048 * 4);
    const unsigned int* ties = (const unsigned int*)(w + M * 4 + (long)N * 2048 * 4 + (long)N * 8);
    const double denom = use_topk ? (double)N * (double)k : (double)M;
    const double per_image = use_topk ? (double)k : (double)HW;
    long blocks = (M / 4 + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    if (C == 5 && ldl == 5 && ldz == 24 && target_is_float && (reinterpret_cast<uintptr_t>(logits) & 7) == 0 &&
        (reinterpret_cast<uintptr_t>(target) & 7) == 0 && (reinterpret_cast<uintptr_t>(dz) & 15) == 0) {
        // the shipped 5-class cfgs (cityscapes-style class list): vector loads / stores
        hipLaunchKernelGGL((seg_ce_bwd_s2d_vec_kernel<5, 24>), dim3(blocks), dim3(256), 0, st, logits, (const float*)target, cw, ignore_index, H, W,
                           M / 4, loss, state, ties, use_topk, gout, (float)(1.0 / denom), (bf16*)dz, valid, per_image);
        HN_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(seg_ce_bwd_s2d_kernel, dim3(blocks), dim3(256), 0, st, logits, ldl, C, target, target_is_float, cw, ignore_index, H, W,
                       M / 4, loss, state, ties, use_topk, gout, (float)(1.0 / denom), (bf16*)dz, ldz, valid, per_image);
    HN_LAUNCH_CHECK();
}
extern "C" int hn_seg_loss_bwd_s2d(const float* logits, int ldl, int C, const void* target, int target_is_float, const float* cw,
                                   int ignore_index, int N, int H, int W, int use_topk, long k, const void* ws, const float* gout, void* dz,
                                   int ldz, hipStream_t st) {
    return seg_loss_bwd_s2d(logits, ldl, C, target, target_is_float, cw, ignore_index, N, H, W, use_topk, k, ws, gout, dz, ldz, nullptr, st);
}
extern "C" int hn_seg_loss_bwd_s2d_masked(const float* logits, int ldl, int C, const void* target, int target_is_float, const float* cw,
                                          int ignore_index, int N, int H, int W, int use_topk, long k, const unsigned char* valid,
                                          const void* ws, const float* gout, void* dz, int ldz, hipStream_t st) {
    HN_CHECK_ARG(valid);
    return seg_loss_bwd_s2d(logits, ldl, C, target, target_is_float, cw, ignore_index, N, H, W, use_topk, k, ws, gout, dz, ldz, valid, st);
}

// ---------------------------------------------------------------------------------------------------------
// Focal variant of the seg loss (head_seg/segmentation_loss.py:31-46, `use_focal: True` of cfgs/hydranet_joint_small_backbone.yml):
//   p = softmax(l) + 1e-8;  t = one_hot(y) + 1e-8;  loss_pix = sum_c t_c * (-alpha * (1 - p_c)^gamma * log(p_c) * w_c);  mean over all pixels
// (every class contributes through the +1e-8 of the one-hot; no ignore_index on this path, as in the reference).
// ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float focal_pow(float q, float gamma) { return gamma == 2.0f ? q * q : powf(q, gamma); }

__global__ __launch_bounds__(256) void seg_focal_fwd_kernel(const float* logits, int ldl, int C, const void* target, int target_is_float,
                                                            const float* cw, float gamma, float alpha, long M, float* psum,
                                                            const unsigned char* valid, long HW) {
    __shared__ float red[4];
    float s = 0.f;
    for (long m = (long)blockIdx.x * 256 + threadIdx.x; m < M; m += (long)gridDim.x * 256) {
        if (valid && !valid[m / HW]) continue;                        // a pixel of an unlabelled image: not in the sum
        const int y = target_is_float ? (int)reinterpret_cast<const float*>(target)[m] : (int)reinterpret_cast<const long*>(target)[m];
        const float* row = logits + m * ldl;
        float mx = row[0];
        for (int c = 1; c < C; ++c) mx = fmaxf(mx, row[c]);
        float e[HN_SEG_MAXC], se = 0.f;
        for (int c = 0; c < C; ++c) { e[c] = expf(row[c] - mx); se += e[c]; }
        float l = 0.f;
        for (int c = 0; c < C; ++c) {
            const float p = e[c] / se + 1e-8f;
            const float t = (c == y ? 1.0f : 0.0f) + 1e-8f;
            l += t * (-alpha * focal_pow(1.0f - p, gamma) * logf(p) * cw[c]);
        }
        s += l;
    }
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) psum[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// dlogits_j = gout/M * s_j * (g_j - sum_c g_c s_c),  g_c = dloss/dp_c = t_c w_c alpha (gamma (1-p_c)^(gamma-1) log p_c - (1-p_c)^gamma / p_c)
__global__ __launch_bounds__(256) void seg_focal_bwd_kernel(const float* logits, int ldl, int C, const void* target, int target_is_float,
                                                            const float* cw, float gamma, float alpha, long M, const float* gout,
                                                            float inv_denom, float* dlogits, int ldd, const unsigned char* valid, long HW) {
    const float gs = gout[0] * (valid ? seg_masked_inv_denom(valid, (int)(M / HW), (double)HW) : inv_denom);
    for (long m = (long)blockIdx.x * 256 + threadIdx.x; m < M; m += (long)gridDim.x * 256) {
        if (valid && !valid[m / HW]) {
            for (int c = 0; c < C; ++c) dlogits[m * ldd + c] = 0.f;
            continue;
        }
        const int y = target_is_float ? (int)reinterpret_cast<const float*>(target)[m] : (int)reinterpret_cast<const long*>(target)[m];
        const float* row = logits + m * ldl;
        float mx = row[0];
        for (int c = 1; c < C; ++c) mx = fmaxf(mx, row[c]);
        float sm[HN_SEG_MAXC], g[HN_SEG_MAXC], se = 0.f, dot = 0.f;
        for (int c = 0; c < C; ++c) { sm[c] = expf(row[c] - mx); se += sm[c]; }
        for (int c = 0; c < C; ++c) {
            sm[c] /= se;
            const float p = sm[c] + 1e-8f, q = 1.0f - p;
            const float t = (c == y ? 1.0f : 0.0f) + 1e-8f;
            const float qg1 = gamma == 2.0f ? q : powf(q, gamma - 1.0f);
            g[c] = t * cw[c] * alpha * (gamma * qg1 * logf(p) - focal_pow(q, gamma) / p);
            dot += g[c] * sm[c];
        }
        float* d = dlogits + m * ldd;
        for (int c = 0; c < C; ++c) d[c] = gs * sm[c] * (g[c] - dot);
    }
}

/* focal seg loss: logits fp32 [N*HW][ldl] (C classes), target float32 or int64 class ids [N*HW] (no ignore_index on this path, as in the
 * reference), ws = fp32 [hn_seg_loss_blocks(N, HW)] partial sums, out[0] = mean over all N*HW pixels */
static int seg_focal_fwd(const float* logits, int ldl, int C, const void* target, int target_is_float, const float* cw, float gamma,
                         float alpha, int N, long HW, void* ws, float* out, const unsigned char* valid, hipStream_t st) {
    HN_CHECK_ARG(logits && target && cw && ws && out && C >= 1 && C <= HN_SEG_MAXC && N > 0 && HW > 0);
    const long M = (long)N * HW;
    const int blocks = hn_seg_loss_blocks(N, HW);
    hipLaunchKernelGGL(seg_focal_fwd_kernel, dim3(blocks), dim3(256), 0, st, logits, ldl, C, target, target_is_float, cw, gamma, alpha, M,
                       (float*)ws, valid, HW);
    hipLaunchKernelGGL(seg_loss_finalize_kernel, dim3(1), dim3(256), 0, st, (const float*)ws, blocks, (const SelState*)nullptr, N, 0, (double)M, out,
                       valid, (double)HW);
    HN_LAUNCH_CHECK();
}
extern "C" int hn_seg_focal_fwd(const float* logits, int ldl, int C, const void* target, int target_is_float, const float* cw, float gamma,
                                float alpha, int N, long HW, void* ws, float* out, hipStream_t st) {
    return seg_focal_fwd(logits, ldl, C, target, target_is_float, cw, gamma, alpha, N, HW, ws, out, nullptr, st);
}
extern "C" int hn_seg_focal_fwd_masked(const float* logits, int ldl, int C, const void* target, int target_is_float, const float* cw,
                                       float gamma, float alpha, int N, long HW, const unsigned char* valid, void* ws, float* out,
                                       hipStream_t st) {
    HN_CHECK_ARG(valid);
    return seg_focal_fwd(logits, ldl, C, target, target_is_float, cw, gamma, alpha, N, HW, ws, out, valid, st);
}

static int seg_focal_bwd(const float* logits, int ldl, int C, const void* target, int target_is_float, const float* cw, float gamma,
                         float alpha, int N, long HW, const float* gout, float* dlogits, int ldd, const unsigned char* valid, hipStream_t st) {
    HN_CHECK_ARG(logits && target && cw && gout && dlogits && C >= 1 && C <= HN_SEG_MAXC && N > 0 && HW > 0);
    const long M = (long)N * HW;
    long blocks = (M + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(seg_focal_bwd_kernel, dim3(blocks), dim3(256), 0, st, logits, ldl, C, target, target_is_float, cw, gamma, alpha, M, gout,
                       (float)(1.0 / (double)M), dlogits, ldd, valid, HW);
    HN_LAUNCH_CHECK();
}
extern "C" int hn_seg_focal_bwd(const float* logits, int ldl, int C, const void* target, int target_is_float, const float* cw, float gamma,
                                float alpha, int N, long HW, const float* gout, float* dlogits, int ldd, hipStream_t st) {
    return seg_focal_bwd(logits, ldl, C, target, target_is_float, cw, gamma, alpha, N, HW, gout, dlogits, ldd, nullptr, st);
}
extern "C" int hn_seg_focal_bwd_masked(const float* logits, int ldl, int C, const void* target, int target_is_float, const float* cw,
                                       float gamma, float alpha, int N, long HW, const unsigned char* valid, const float* gout,
                                       float* dlogits, int ldd, hipStream_t st) {
    HN_CHECK_ARG(valid);
    return seg_focal_bwd(logits, ldl, C, target, target_is_float, cw, gamma, alpha, N, HW, gout, dlogits, ldd, valid, st);
}

extern "C" int hn_argmax_channels(const float* logits, int ldl, int C, long M, long* out, hipStream_t st) {
    HN_CHECK_ARG(logits && out && C >= 1 && M > 0);
    long blocks = (M + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(argmax_kernel, dim3(blocks), dim3(256), 0, st, logits, ldl, C, M, out);
    HN_LAUNCH_CHECK();
}

// ---------------------------------------------------------------------------------------------------------
// Lane losses (head_lane/lanedetect_loss.py:5-78): OHEM classification loss and masked Huber location loss.
//   cls: M = N*hw anchors, logits [M][2], target one-hot [M][2] (positive = t[1] > 0).  NEGATIVE_RATIO 15, ALPHA 10.
//        neg_num = clamp(15 * #pos, 1, #neg); thr = neg_num-th smallest background log-prob among the negatives (detached);
//        pos = -alpha * sum_{pos} log p_fg / max(#pos,1);  neg = -alpha * sum_{neg, log p_bg <= thr} log p_bg / max(#pos,1)
//   One workgroup of 1024 threads does the whole problem (M is 8 192 at batch 16): log-softmax, counts, a 4-pass byte radix select of the
//   k-th smallest value in LDS histograms (instead of torch.sort), and both sums.  aux[0..3] = {thr, max(#pos,1), #pos, #neg}.
// ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned int f2ord(float f) {              // order-preserving float -> uint
    const unsigned int u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ord2f(unsigned int o) {
    const unsigned int u = (o & 0x80000000u) ? (o & 0x7fffffffu) : ~o;
    return __uint_as_float(u);
}
// k-th element's bin of a 256-bin LDS histogram, found by all threads together: thread b < 256 takes bin b, an inclusive prefix sum runs
// inside each of the four waves (shuffles) and across them (LDS), and the one thread whose bin satisfies excl < k <= incl publishes
// (bin, k - excl).  (One thread walking the 256 bins was ~10 us per radix pass: 256 dependent LDS reads.)  All 1024 threads call it.
__device__ __forceinline__ void hist_select_256(const unsigned int* hist, unsigned int k, unsigned int* wsum /* [4] LDS */, unsigned int* out_bin,
                                                unsigned int* out_k) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned int v = tid < 256 ? hist[tid] : 0u, incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned int t = __shfl_up(incl, d);
        if (lane >= d) incl += t;
    }
    if (tid < 256 && lane == 63) wsum[wave] = incl;
    __syncthreads();
    if (tid < 256) {
        unsigned int base = 0;
        for (int w2 = 0; w2 < wave; ++w2) base += wsum[w2];
        incl += base;
        const unsigned int excl = incl - v;
        if (excl < k && k <= incl) { *out_bin = (unsigned int)tid; *out_k = k - excl; }
    }
    __syncthreads();
}
// With a mask (valid: the lane row of the task masks, R rows per image) the rows of an unlabelled image are neither positive nor negative:
// their log-probabilities are still written, but they stay out of the counts, the rank, the select and both sums.
__device__ __forceinline__ bool lane_row_valid(const unsigned char* valid, int R, long i) { return !valid || valid[(int)i / R] != 0; }

__global__ __launch_bounds__(1024) void lane_cls_fwd_kernel(const float* logits, const float* target, long M, float neg_ratio, float alpha,
                                                            float* lsm, unsigned char* pmask, float* out, float* aux,
                                                            const unsigned char* valid, int R) {
    __shared__ unsigned int hist[256];
    __shared__ float red[16];
    __shared__ unsigned int s_bin, s_k, s_wsum[4];
    const int tid = threadIdx.x;
    float npos = 0.f, nneg = 0.f;
    for (long i = tid; i < M; i += 1024) {
        const float z0 = logits[2 * i], z1 = logits[2 * i + 1];
        const float mx = fmaxf(z0, z1);
        const float lse = mx + logf(expf(z0 - mx) + expf(z1 - mx));
        lsm[2 * i] = z0 - lse;
        lsm[2 * i + 1] = z1 - lse;
        const bool ok = lane_row_valid(valid, R, i);
        const bool p = ok && target[2 * i + 1] > 0.f;
        pmask[i] = p ? 1 : 0;
        npos += p ? 1.f : 0.f;
        nneg += p || !ok ? 0.f : 1.f;
    }
    npos = block_sum_1024(npos, red);
    nneg = block_sum_1024(nneg, red);
    const float posn = fmaxf(npos, 1.f);
    long kk = (long)fmaxf(fminf(npos * neg_ratio, nneg), 1.f);       // 1-based rank among the negatives
    float thr = __builtin_inff();
    if (nneg >= 1.f) {
        // byte-wise radix select, most significant byte first, over the order-preserving keys of the negatives' background log-probs
        unsigned int prefix = 0, k = (unsigned int)kk;
        for (int pass = 0; pass < 4; ++pass) {
            const int shift = 24 - 8 * pass;
            if (tid < 256) hist[tid] = 0;
            __syncthreads();
            const unsigned int himask = pass == 0 ? 0u : (0xffffffffu << (shift + 8));
            for (long i = tid; i < M; i += 1024) {
                if (pmask[i] || !lane_row_valid(valid, R, i)) continue;
                const unsigned int key = f2ord(lsm[2 * i]);
                if ((key & himask) == prefix) atomicAdd(&hist[(key >> shift) & 255], 1u);
            }
            __syncthreads();
            hist_select_256(hist, k, s_wsum, &s_bin, &s_k);
            prefix |= s_bin << shift;
            k = s_k;
        }
        thr = ord2f(prefix);
    }
    float sp = 0.f, sn = 0.f;
    for (long i = tid; i < M; i += 1024) {
        const float bg = lsm[2 * i], fg = lsm[2 * i + 1];
        if (pmask[i]) sp += fg;
        else if (bg <= thr && lane_row_valid(valid, R, i)) sn += bg;
    }
    sp = block_sum_1024(sp, red);
    sn = block_sum_1024(sn, red);
    if (tid == 0) {
        out[0] = -alpha * sp / posn;
        out[1] = -alpha * sn / posn;
        aux[0] = thr; aux[1] = posn; aux[2] = npos; aux[3] = nneg;
    }
}
// The same selection with every row held in registers (M <= 1024 * RPT): the seven passes of the kernel above each made a global-memory
// round trip over the rows with one workgroup (58 us for 32 768 rows); here the rows are read once, the radix passes run on registers.
template <int RPT>
__global__ __launch_bounds__(1024) void lane_cls_fwd_reg_kernel(const float* logits, const float* target, long M, float neg_ratio, float alpha,
                                                                float* lsm, unsigned char* pmask, float* out, float* aux,
                                                                const unsigned char* vmask, int R) {
    __shared__ unsigned int hist[256];
    __shared__ float red[16];
    __shared__ unsigned int s_bin, s_k, s_wsum[4];
    const int tid = threadIdx.x;
    float bg[RPT], fg[RPT];
    unsigned int pos = 0, valid = 0;                                  // bit j: row tid + 1024 j is a positive / exists (and is labelled)
    float npos = 0.f, nneg = 0.f;
#pragma unroll
    for (int j0 = 0; j0 < RPT; j0 += 8) {                              // eight rows' loads in flight at a time
        float2 zz[8], tt[8];
#pragma unroll
        for (int jj = 0; jj < 8; ++jj) {
            const long i = tid + 1024L * (j0 + jj);
            zz[jj] = make_float2(0.f, 0.f); tt[jj] = make_float2(0.f, 0.f);
            if (i < M) {
                zz[jj] = *reinterpret_cast<const float2*>(logits + 2 * i);
                tt[jj] = *reinterpret_cast<const float2*>(target + 2 * i);
            }
        }
#pragma unroll
        for (int jj = 0; jj < 8; ++jj) {
            const int j = j0 + jj;
            const long i = tid + 1024L * j;
            const float z0 = zz[jj].x, z1 = zz[jj].y;
            const float mx = fmaxf(z0, z1);
            const float lse = mx + logf(expf(z0 - mx) + expf(z1 - mx));
            bg[j] = z0 - lse;
            fg[j] = z1 - lse;
            if (i < M) {
                const bool ok = lane_row_valid(vmask, R, i);
                const bool p = ok && tt[jj].y > 0.f;
                valid |= ok ? (1u << j) : 0u;
                pos |= p ? (1u << j) : 0u;
                *reinterpret_cast<float2*>(lsm + 2 * i) = make_float2(bg[j], fg[j]);
                pmask[i] = p ? 1 : 0;
                npos += p ? 1.f : 0.f;
                nneg += p || !ok ? 0.f : 1.f;
            }
        }
    }
    npos = block_sum_1024(npos, red);
    nneg = block_sum_1024(nneg, red);
    const float posn = fmaxf(npos, 1.f);
    long kk = (long)fmaxf(fminf(npos * neg_ratio, nneg), 1.f);
    float thr = __builtin_inff();
    const unsigned int negs = valid & ~pos;
    if (nneg >= 1.f) {
        unsigned int prefix = 0, k = (unsigned int)kk;
        for (int pass = 0; pass < 4; ++pass) {
            const int shift = 24 - 8 * pass;
            if (tid < 256) hist[tid] = 0;
            __syncthreads();
            const unsigned int himask = pass == 0 ? 0u : (0xffffffffu << (shift + 8));
#pragma unroll
            for (int j = 0; j < RPT; ++j) {
                if (!((negs >> j) & 1u)) continue;
                const unsigned int key = f2ord(bg[j]);
                if ((key & himask) == prefix) atomicAdd(&hist[(key >> shift) & 255], 1u);
            }
            __syncthreads();
            hist_select_256(hist, k, s_wsum, &s_bin, &s_k);
            prefix |= s_bin << shift;
            k = s_k;
        }
        thr = ord2f(prefix);
    }
    float sp = 0.f, sn = 0.f;
#pragma unroll
    for (int j = 0; j < RPT; ++j) {
        if ((pos >> j) & 1u) sp += fg[j];
        else if (((negs >> j) & 1u) && bg[j] <= thr) sn += bg[j];
    }
    sp = block_sum_1024(sp, red);
    sn = block_sum_1024(sn, red);
    if (tid == 0) {
        out[0] = -alpha * sp / posn;
        out[1] = -alpha * sn / posn;
        aux[0] = thr; aux[1] = posn; aux[2] = npos; aux[3] = nneg;
    }
}
// dlogits = gpos * d(pos)/dz + gneg * d(neg)/dz
__global__ void lane_cls_bwd_kernel(const float* lsm, const unsigned char* pmask, const float* aux, const float* gpos, const float* gneg,
                                    float alpha, long M, float* dlogits, const unsigned char* valid, int R) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M) return;
    const float thr = aux[0], posn = aux[1];
    const float bg = lsm[2 * i], fg = lsm[2 * i + 1];
    const float p0 = expf(bg), p1 = expf(fg);
    float d0 = 0.f, d1 = 0.f;
    if (pmask[i]) {                                    // -alpha/P * log p_fg
        const float c = -alpha / posn * gpos[0];
        d0 = -p0 * c;
        d1 = (1.f - p1) * c;
    } else if (bg <= thr && lane_row_valid(valid, R, i)) {   // -alpha/P * log p_bg
        const float c = -alpha / posn * gneg[0];
        d0 = (1.f - p0) * c;
        d1 = -p1 * c;
    }
    dlogits[2 * i] = d0;
    dlogits[2 * i + 1] = d1;
}
// location loss: per row r (positive anchors only): sum_c huber(p - t) * w_c * [t != 0] / max(#[t != 0], 1); w = alpha at columns wcol, wcol+1.
// block = 8 rows x 32 lanes; rowloss[r] (0 for negatives) and the per-row normaliser go to workspace; a 1-block finalize sums the rows.
__global__ __launch_bounds__(256) void lane_loc_fwd_kernel(const float* pred, const float* tgt, const unsigned char* pmask, long M, int L,
                                                           int wcol, float alpha, float* rowloss, float* rownorm) {
    const int lane = threadIdx.x & 31, rr = threadIdx.x >> 5;
    const long r = (long)blockIdx.x * 8 + rr;
    float s = 0.f, cnt = 0.f;
    if (r < M) {
        const bool pos = pmask[r] != 0;
        for (int c = lane; c < L; c += 32) {
            const float t = tgt[r * L + c];
            if (t != 0.f) {
                cnt += 1.f;
                if (pos) {
                    const float d = pred[r * L + c] - t, ad = fabsf(d);
                    const float hv = ad < 1.f ? 0.5f * d * d : ad - 0.5f;
                    s += hv * ((c == wcol || c == wcol + 1) ? alpha : 1.f);
                }
            }
        }
    }
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) { s += __shfl_xor(s, o); cnt += __shfl_xor(cnt, o); }
    if (lane == 0 && r < M) {
        const float nrm = fmaxf(cnt, 1.f);
        rownorm[r] = nrm;
        rowloss[r] = s / nrm;
    }
}
__global__ __launch_bounds__(1024) void lane_loc_finalize_kernel(const float* rowloss, long M, const float* aux, float* out) {
    __shared__ float red[16];
    float s = 0.f;
    for (long i = threadIdx.x; i < M; i += 1024) s += rowloss[i];
    s = block_sum_1024(s, red);
    if (threadIdx.x == 0) out[0] = s / aux[1];
}
__global__ void lane_loc_bwd_kernel(const float* pred, const float* tgt, const unsigned char* pmask, const float* rownorm, const float* aux,
                                    const float* gout, long M, int L, int wcol, float alpha, float* dpred) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= M * L) return;
    const long r = idx / L;
    const int c = (int)(idx - r * L);
    float g = 0.f;
    const float t = tgt[idx];
    if (pmask[r] && t != 0.f) {
        const float d = pred[idx] - t;
        const float dh = fabsf(d) < 1.f ? d : (d > 0.f ? 1.f : -1.f);
        g = dh * ((c == wcol || c == wcol + 1) ? alpha : 1.f) / rownorm[r] / aux[1] * gout[0];
    }
    dpred[idx] = g;
}

static int lane_cls_loss_fwd(const float* logits, const float* target, long M, float neg_ratio, float alpha, float* lsm,
                             void* pmask, float* out, float* aux, const unsigned char* valid, int R, hipStream_t st) {
    HN_CHECK_ARG(logits && target && lsm && pmask && out && aux && M > 0 && M <= (1L << 22));
    const bool al8 = ((reinterpret_cast<uintptr_t>(logits) | reinterpret_cast<uintptr_t>(target) | reinterpret_cast<uintptr_t>(lsm)) & 7) == 0;
    if (al8 && M <= 1024L * 8)
        hipLaunchKernelGGL(lane_cls_fwd_reg_kernel<8>, dim3(1), dim3(1024), 0, st, logits, target, M, neg_ratio, alpha, lsm, (unsigned char*)pmask, out, aux, valid, R);
    else if (al8 && M <= 1024L * 32)
        hipLaunchKernelGGL(lane_cls_fwd_reg_kernel<32>, dim3(1), dim3(1024), 0, st, logits, target, M, neg_ratio, alpha, lsm, (unsigned char*)pmask, out, aux, valid, R);
    else
        hipLaunchKernelGGL(lane_cls_fwd_kernel, dim3(1), dim3(1024), 0, st, logits, target, M, neg_ratio, alpha, lsm, (unsigned char*)pmask, out, aux, valid, R);
    HN_LAUNCH_CHECK();
}
extern "C" int hn_lane_cls_loss_fwd(const float* logits, const float* target, long M, float neg_ratio, float alpha, float* lsm,
                                    void* pmask, float* out, float* aux, hipStream_t st) {
    return lane_cls_loss_fwd(logits, target, M, neg_ratio, alpha, lsm, pmask, out, aux, nullptr, 1, st);
}
/* rows: rows per image (M = N x rows); valid: uint8 [N] */
extern "C" int hn_lane_cls_loss_fwd_masked(const float* logits, const float* target, long M, int rows, const unsigned char* valid,
                                           float neg_ratio, float alpha, float* lsm, void* pmask, float* out, float* aux, hipStream_t st) {
    HN_CHECK_ARG(valid && rows > 0 && M > 0 && M % rows == 0);
    return lane_cls_loss_fwd(logits, target, M, neg_ratio, alpha, lsm, pmask, out, aux, valid, rows, st);
}
static int lane_cls_loss_bwd(const float* lsm, const void* pmask, const float* aux, const float* gpos, const float* gneg, float alpha,
                             long M, float* dlogits, const unsigned char* valid, int R, hipStream_t st) {
    HN_CHECK_ARG(lsm && pmask && aux && gpos && gneg && dlogits && M > 0);
    hipLaunchKernelGGL(lane_cls_bwd_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, st, lsm, (const unsigned char*)pmask, aux, gpos, gneg,
                       alpha, M, dlogits, valid, R);
    HN_LAUNCH_CHECK();
}
extern "C" int hn_lane_cls_loss_bwd(const float* lsm, const void* pmask, const float* aux, const float* gpos, const float* gneg, float alpha,
                                    long M, float* dlogits, hipStream_t st) {
    return lane_cls_loss_bwd(lsm, pmask, aux, gpos, gneg, alpha, M, dlogits, nullptr, 1, st);
}
extern "C" int hn_lane_cls_loss_bwd_masked(const float* lsm, const void* pmask, const float* aux, const float* gpos, const float* gneg,
                                           float alpha, long M, int rows, const unsigned char* valid, float* dlogits, hipStream_t st) {
    HN_CHECK_ARG(valid && rows > 0 && M > 0 && M % rows == 0 && M <= (1L << 22));
    return lane_cls_loss_bwd(lsm, pmask, aux, gpos, gneg, alpha, M, dlogits, valid, rows, st);
}
extern "C" int hn_lane_loc_loss_fwd(const float* pred, const float* target, const void* pmask, const float* aux, long M, int L, int wcol,
                                    float alpha, float* rowloss, float* rownorm, float* out, hipStream_t st) {
    HN_CHECK_ARG(pred && target && pmask && aux && rowloss && rownorm && out && M > 0 && L > 0 && wcol >= 0 && wcol + 1 < L);
    hipLaunchKernelGGL(lane_loc_fwd_kernel, dim3((unsigned)((M + 7) / 8)), dim3(256), 0, st, pred, target, (const unsigned char*)pmask, M, L, wcol,
                       alpha, rowloss, rownorm);
    hipLaunchKernelGGL(lane_loc_finalize_kernel, dim3(1), dim3(1024), 0, st, rowloss, M, aux, out);
    HN_LAUNCH_CHECK();
}
extern "C" int hn_lane_loc_loss_bwd(const float* pred, const float* target, const void* pmask, const float* rownorm, const float* aux,
                                    const float* gout, long M, int L, int wcol, float alpha, float* dpred, hipStream_t st) {
    HN_CHECK_ARG(pred && target && pmask && rownorm && aux && gout && dpred && M > 0 && L > 0);
    hipLaunchKernelGGL(lane_loc_bwd_kernel, dim3((unsigned)((M * L + 255) / 256)), dim3(256), 0, st, pred, target, (const unsigned char*)pmask,
                       rownorm, aux, gout, M, L, wcol, alpha, dpred);
    HN_LAUNCH_CHECK();
}

// ---------------------------------------------------------------------------------------------------------
// Device NMS for the detection post-process (head_detect/detection_loss.py:70-108; torchvision.ops.batched_nms semantics restated in
// postprocess.py): boxes are already sorted by descending score (stable) and carry their class offset.
//   nms_mask_kernel: bit (i, j) of mask[i][j/64] = (j > i) and IoU(i, j) > thr, IoU = inter / (area_i + area_j - inter) in separately
//                    rounded fp32 operations (no FMA contraction), so the comparisons are bit-identical to the numpy/torch host path;
//   nms_scan_kernel: one wave walks the boxes in order, keeps box i unless an earlier kept box suppressed it (64-bit word per lane).
// ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float iou_rn(const float4 a, const float4 b) {
    const float area_a = __fmul_rn(__fsub_rn(a.z, a.x), __fsub_rn(a.w, a.y));
    const float area_b = __fmul_rn(__fsub_rn(b.z, b.x), __fsub_rn(b.w, b.y));
    float iw = __fsub_rn(fminf(a.z, b.z), fmaxf(a.x, b.x));
    float ih = __fsub_rn(fminf(a.w, b.w), fmaxf(a.y, b.y));
    iw = iw > 0.f ? iw : 0.f;
    ih = ih > 0.f ? ih : 0.f;
    const float inter = __fmul_rn(iw, ih);
    return __fdiv_rn(inter, __fsub_rn(__fadd_rn(area_a, area_b), inter));
}
__global__ __launch_bounds__(64) void nms_mask_kernel(const float4* boxes, int K, float thr, unsigned long long* mask, int words) {
    const int i = blockIdx.y;                         // row box
    const int wj = blockIdx.x;                        // 64-column word
    const int j = wj * 64 + threadIdx.x;
    bool sup = false;
    if (j < K && j > i) sup = iou_rn(boxes[i], boxes[j]) > thr;
    const unsigned long long bits = __ballot(sup);
    if (threadIdx.x == 0) mask[(long)i * words + wj] = bits;
}
__global__ __launch_bounds__(64) void nms_scan_kernel(const unsigned long long* mask, int K, int words, unsigned char* keep) {
    // lane l owns removed-words l, l+64, ...  (K <= 64 * 64 * NW)
    constexpr int NW = 8;
    unsigned long long removed[NW];
#pragma unroll
    for (int w = 0; w < NW; ++w) removed[w] = 0ull;
    const int lane = threadIdx.x;
    for (int i = 0; i < K; ++i) {
        const int wi = i >> 6;
        // is box i still alive?  its bit lives in word wi, owned by lane wi % 64, slot wi / 64
        unsigned long long wv = 0ull;
#pragma unroll
        for (int w = 0; w < NW; ++w) if ((wi >> 6) == w) wv = removed[w];
        const unsigned long long word = __shfl(wv, wi & 63);
        const bool alive = !((word >> (i & 63)) & 1ull);
        if (lane == 0) keep[i] = alive ? 1 : 0;
        if (alive) {
#pragma unroll
            for (int w = 0; w < NW; ++w) {
                const int ww = w * 64 + lane;
                if (ww < words) removed[w] |= mask[(long)i * words + ww];
            }
        }
    }
}
extern "C" long hn_nms_mask_words(int K) { return (long)K * ((K + 63) / 64); }
/* boxes: fp32 [K][4] (x1, y1, x2, y2), sorted by descending score, class offsets already added; mask: hn_nms_mask_words(K) uint64;
 * keep: K bytes (1 = kept).  K <= 32768. */
extern "C" int hn_nms_sorted(const float* boxes, int K, float iou_threshold, void* mask, void* keep, hipStream_t st) {
    HN_CHECK_ARG(boxes && mask && keep && K > 0 && K <= 32768);
    const int words = (K + 63) / 64;
    hipLaunchKernelGGL(nms_mask_kernel, dim3(words, K), dim3(64), 0, st, (const float4*)boxes, K, iou_threshold, (unsigned long long*)mask, words);
    hipLaunchKernelGGL(nms_scan_kernel, dim3(1), dim3(64), 0, st, (const unsigned long long*)mask, K, words, (unsigned char*)keep);
    HN_LAUNCH_CHECK();
}

// ---------------------------------------------------------------------------------------------------------
// Weighted multitask loss sum (HydraTrainer.cal_total_loss, model/train.py:192-203) in one launch:
//   total = sum_g ( sum_{i in g} x_i * w_i ) * gw_g        evaluated left to right in fp32, no fused multiply-add (the reference's separate
//   mul / add kernels round after every operation); backward: dx_i = (gout * gw_g) * w_i
// ---------------------------------------------------------------------------------------------------------
#define HN_MAX_LOSS_TERMS 8
struct WSum {
    const float* x[HN_MAX_LOSS_TERMS]; float w[HN_MAX_LOSS_TERMS]; float gw[HN_MAX_LOSS_TERMS]; int grp[HN_MAX_LOSS_TERMS];
    int n; const float* gout; float* out; float* grads;
};
// (plain operators under the pragma, as ema_lerp_rn in hn_common.h: written with __fadd_rn(s, __fmul_rn(x, w)) every product was
// contracted into the sum that takes it, one rounding instead of two, and the total differed from the reference's in the last bit)
__global__ void weighted_sum_kernel(const WSum p) {
#pragma clang fp contract(off)
    if (threadIdx.x != 0) return;
    if (p.out) {
        float tot = 0.f;
        int i = 0;
        while (i < p.n) {
            const int g = p.grp[i];
            float s = p.x[i][0] * p.w[i];
            for (++i; i < p.n && p.grp[i] == g; ++i) {
                const float t = p.x[i][0] * p.w[i];
                s = s + t;
            }
            const float sg = s * p.gw[g];
            tot = tot + sg;
        }
        p.out[0] = tot;
    }
    if (p.grads) {
        const float go = p.gout[0];
        for (int i = 0; i < p.n; ++i) {
            const float gg = go * p.gw[p.grp[i]];
            p.grads[i] = gg * p.w[i];
        }
    }
}
/* xs: HOST array of n device pointers (one fp32 scalar each); w, gw, grp: HOST arrays (term weight, group weight indexed by group id, group
 * id per term; terms of a group are consecutive); out (optional): the total; grads (optional, with gout): n gradients */
extern "C" int hn_weighted_sum(const void* const* xs, const float* w, const float* gw, const int* grp, int n, const float* gout, float* out,
                               float* grads, hipStream_t st) {
    HN_CHECK_ARG(xs && w && gw && grp && n > 0 && n <= HN_MAX_LOSS_TERMS && (out || grads) && (!grads || gout));
    WSum p = {};
    for (int i = 0; i < n; ++i) {
        HN_CHECK_ARG(xs[i] && grp[i] >= 0 && grp[i] < HN_MAX_LOSS_TERMS && (i == 0 || grp[i] >= grp[i - 1]));
        p.x[i] = (const float*)xs[i]; p.w[i] = w[i]; p.grp[i] = grp[i];
    }
    for (int g = 0; g <= grp[n - 1]; ++g) p.gw[g] = gw[g];
    p.n = n; p.gout = gout; p.out = out; p.grads = grads;
    hipLaunchKernelGGL(weighted_sum_kernel, dim3(1), dim3(64), 0, st, p);
    HN_LAUNCH_CHECK();
}

// ---------------------------------------------------------------------------------------------------------
// The same sum under learned homoscedastic-uncertainty weights (Kendall, Gal and Cipolla, CVPR 2018; train.loss_balance): one
// log-variance s per term, clamped to [-S, S],
//   e_i = expf(-s~_i)     t_i = (x_i * w_i) * e_i     total = [ sum_g ( sum_{i in g} t_i ) * gw_g ] + sum_{i active} s~_i
// the bracket in weighted_sum_kernel's order, the regulariser added last in term order, every operation rounded on its own.  A term is
// ACTIVE when x_i != 0 (a masked task, a head without positives): an inactive term adds neither t_i nor s~_i and its ds is 0 -- ds = 1
// would push s down without bound.  Backward: dx_i = ((gout * gw_g) * w_i) * e_i; ds_i = gout * (1 - t_i * gw_g) inside the clamp, and at
// or outside it only when a descent step (s -= lr * ds) moves s back inside.  At s = 0: expf(0) = 1, x * 1 and + 0 are exact, so total
// and every dx_i are weighted_sum_kernel's bits.
// record (fp32 [2 * HN_MAX_LOSS_TERMS], by term): e_i, then 1.0 / 0.0 = active; ds (fp32 [2 * n_slots], by slot): the gradient, then
// 1.0 / 0.0 = the slot's term was active.  Every entry is written: an unused one as 0.0.
// ---------------------------------------------------------------------------------------------------------
struct BSum {
    WSum ws; int slot[HN_MAX_LOSS_TERMS]; int n_slots; const float* s; float clamp; float* record; float* ds;
};
__global__ void balanced_sum_kernel(const BSum p) {
#pragma clang fp contract(off)
    if (threadIdx.x != 0) return;
    const WSum& q = p.ws;
    float e[HN_MAX_LOSS_TERMS], sc[HN_MAX_LOSS_TERMS], x[HN_MAX_LOSS_TERMS];
    bool act[HN_MAX_LOSS_TERMS];
#pragma unroll
    for (int i = 0; i < HN_MAX_LOSS_TERMS; ++i) {
        e[i] = 0.f; sc[i] = 0.f; x[i] = 0.f; act[i] = false;
        if (i < q.n) {
            x[i] = q.x[i][0];
            act[i] = x[i] != 0.f;
            sc[i] = fminf(fmaxf(p.s[p.slot[i]], -p.clamp), p.clamp);
            if (q.out) e[i] = expf(-sc[i]);
            else e[i] = p.record[i];                        // backward alone: the forward's multipliers
        }
    }
    if (q.out) {
        float tot = 0.f;
        int i = 0;
        while (i < q.n) {
            const int g = q.grp[i];
            float s = 0.f;
            bool first = true;
            for (; i < q.n && q.grp[i] == g; ++i) {
                if (!act[i]) continue;
                const float xw = x[i] * q.w[i];
                const float t = xw * e[i];
                s = first ? t : s + t;
                first = false;
            }
            const float sg = s * q.gw[g];
            tot = tot + sg;
        }
        for (int i = 0; i < q.n; ++i)
            if (act[i]) tot = tot + sc[i];
        q.out[0] = tot;
#pragma unroll
        for (int i = 0; i < HN_MAX_LOSS_TERMS; ++i) {
            p.record[i] = i < q.n ? e[i] : 0.f;
            p.record[HN_MAX_LOSS_TERMS + i] = (i < q.n && act[i]) ? 1.f : 0.f;
        }
    }
    if (q.grads) {
        const float go = q.gout[0];
        for (int k = 0; k < 2 * p.n_slots; ++k) p.ds[k] = 0.f;
        for (int i = 0; i < q.n; ++i) {
            const float gwi = q.gw[q.grp[i]];
            const float gg = go * gwi;
            const float gw_ = gg * q.w[i];
            q.grads[i] = gw_ * e[i];                        // (also of an inactive term: at s = 0 the parent's seed, whatever x_i is)
            if (!act[i]) continue;
            const float xw = x[i] * q.w[i];
            const float t = xw * e[i];
            const float u = t * gwi;
            const float v = 1.f - u;
            const float d = go * v;
            const float sv = p.s[p.slot[i]];
            const bool keep = (sv > -p.clamp && sv < p.clamp) || (sv >= p.clamp && d > 0.f) || (sv <= -p.clamp && d < 0.f);
            p.ds[p.slot[i]] = keep ? d : 0.f;
            p.ds[p.n_slots + p.slot[i]] = 1.f;
        }
    }
}
/* hn_weighted_sum's arguments, plus: slot (HOST, [n], strictly increasing, < n_slots <= 8): the entry of s / ds that term i owns; s (DEVICE
 * fp32 [n_slots]): the log-variances, read at the n slots only; clamp = S > 0; record (DEVICE fp32 [16], always): written by a forward
 * call, read by a call without `out`; ds (DEVICE fp32 [2 * n_slots], with grads). */
extern "C" int hn_balanced_sum(const void* const* xs, const float* w, const float* gw, const int* grp, const int* slot, int n, int n_slots,
                               const float* s, float clamp, const float* gout, float* out, float* record, float* grads, float* ds,
                               hipStream_t st) {
    HN_CHECK_ARG(xs && w && gw && grp && slot && n > 0 && n <= HN_MAX_LOSS_TERMS && n_slots >= n && n_slots <= HN_MAX_LOSS_TERMS);
    HN_CHECK_ARG(s && record && clamp > 0.f && clamp <= 80.f && (out || grads) && (!grads || (gout && ds)));
    BSum p = {};
    for (int i = 0; i < n; ++i) {
        HN_CHECK_ARG(xs[i] && grp[i] >= 0 && grp[i] < HN_MAX_LOSS_TERMS && (i == 0 || grp[i] >= grp[i - 1]));
        HN_CHECK_ARG(slot[i] >= 0 && slot[i] < n_slots && (i == 0 || slot[i] > slot[i - 1]));
        p.ws.x[i] = (const float*)xs[i]; p.ws.w[i] = w[i]; p.ws.grp[i] = grp[i]; p.slot[i] = slot[i];
    }
    for (int g = 0; g <= grp[n - 1]; ++g) p.ws.gw[g] = gw[g];
    p.ws.n = n; p.ws.gout = gout; p.ws.out = out; p.ws.grads = grads;
    p.n_slots = n_slots; p.s = s; p.clamp = clamp; p.record = record; p.ds = ds;
    hipLaunchKernelGGL(balanced_sum_kernel, dim3(1), dim3(64), 0, st, p);
    HN_LAUNCH_CHECK();
}

// Adam steps every element of the log-variance tensor; a slot whose term was inactive (or is not trained in this phase) must keep s and
// both moments to the bit.  hold (fp32 [3 * n]): act == nullptr copies s, m, v into it (before the step); otherwise slot i is written
// back from it where !(act[i] > 0) (after the step; act = the ds vector's second half, or its mean over a group of micro-batches).
__global__ void balance_hold_kernel(float* s, float* m, float* v, float* hold, const float* act, int n) {
    const int i = threadIdx.x;
    if (i >= n) return;
    if (!act) { hold[i] = s[i]; hold[n + i] = m[i]; hold[2 * n + i] = v[i]; return; }
    if (!(act[i] > 0.f)) { s[i] = hold[i]; m[i] = hold[n + i]; v[i] = hold[2 * n + i]; }
}
extern "C" int hn_balance_hold(float* s, float* m, float* v, float* hold, const float* act, int n, hipStream_t st) {
    HN_CHECK_ARG(s && m && v && hold && n > 0 && n <= HN_MAX_LOSS_TERMS);
    hipLaunchKernelGGL(balance_hold_kernel, dim3(1), dim3(64), 0, st, s, m, v, hold, act, n);
    HN_LAUNCH_CHECK();
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Adam step of ALL parameters in one launch (torch.optim.Adam as the reference constructs it, model/train.py:147: L2 weight decay added to
// the gradient, bias-corrected moments, eps outside the square root).  The foreach implementation is ~10 launches over 693 tensor lists
// (3.9 ms per step on the big cfg); this is one pass over p, g, m, v (1.2 GB: ~0.35 ms).  jobs (device): n x {p, g, m, v, numel,
// first_block}; a block = 256 threads x 4 consecutive elements; block_job: job index of every block.
// Same operation order as torch's single-tensor formula (lerp for the first moment, mul + addcmul for the second, sqrt / bias2_sqrt +
// eps, addcdiv), with explicitly rounded steps (no fused multiply-add), so that it tracks torch.optim.Adam to the last bit or two.
// ---------------------------------------------------------------------------------------------------------------------------------
// The step's decision, written by hn_grad_guard (below) and obeyed by hn_adam_step_guarded: 32 bytes on the device, zeroed once by the caller.
struct GuardRecord { float norm, coef; int skip, steps, skipped, skipped_consecutive, pad[2]; };

// (the average's update, ema_lerp_rn: hn_common.h)

// GUARDED = false is hn_adam_step.  GUARDED = true (hn_adam_step_guarded) reads the record first: a flagged step returns before its first
// store; otherwise the gradient is scaled by the clipping coefficient before the weight-decay term, i.e. clip in place, then step --
// without writing the gradient.  x * 1.0f == x, so coef == 1.0f gives hn_adam_step's bits.
// EMA = true (hn_adam_step_ema) also keeps an exponential moving average e of the parameter (ema: one fp32 pointer per job): once the new
// parameter value p' is in its register, e' = e + w * (p' - e) in rounded operations -- one more read and one more write per element, no
// second pass over p.  p, m and v are formed by the same instructions as without it; a skipped step leaves e untouched as well.
template <bool GUARDED, bool EMA>
__global__ __launch_bounds__(256) void adam_step_kernel(const long* jobs, const int* block_job, float lr_over_bc1, float w1, float b2, float w2,
                                                        float eps, float wd, float bc2_sqrt, const GuardRecord* rec, const long* ema,
                                                        float ema_w) {
    float coef = 1.f;
    if constexpr (GUARDED) {
        if (rec->skip != 0) return;
        coef = rec->coef;
    }
    const int job = block_job[blockIdx.x];
    const long* jb = jobs + (long)job * 6;
    float* e = nullptr;
    if constexpr (EMA) e = reinterpret_cast<float*>(ema[job]);
    float* p = reinterpret_cast<float*>(jb[0]);
    const float* g = reinterpret_cast<const float*>(jb[1]);
    float* m = reinterpret_cast<float*>(jb[2]);
    float* v = reinterpret_cast<float*>(jb[3]);
    const long n = jb[4];
    const long i0 = (((long)blockIdx.x - jb[5]) * 256 + threadIdx.x) * 4;
    if (i0 >= n) return;
    // Every operation below is rounded on its own: plain operators under contract(off), one per statement, and the correctly rounded
    // square root.  (The __f*_rn intrinsics do not give that here: to this compiler __fmul_rn / __fadd_rn are the plain operators under
    // HIP's default -ffp-contract=fast-honor-pragmas -- the four product-and-sum pairs below compiled to v_pk_fma_f32 -- and __fsqrt_rn is
    // the native v_sqrt_f32 without its refinement; ema_lerp_rn in hn_common.h met the same.  tests/adam_ref.py restates the sequence in
    // numpy float32 and tests/test_adam_exact_gpu.py holds p, m and v to it bit for bit.)
    auto one = [&](float pv, float gv, float& mv, float& vv) {
#pragma clang fp contract(off)
        if constexpr (GUARDED) gv = gv * coef;                                         // clip_grad_norm_'s grad.mul_(clip_coef), not stored
        if (wd != 0.f) { const float t = wd * pv; gv = gv + t; }
        const float d = gv - mv, t1 = w1 * d;
        mv = mv + t1;                                                                  // exp_avg.lerp_(grad, 1 - beta1)
        const float g2 = gv * gv, t2 = w2 * g2, t3 = vv * b2;
        vv = t3 + t2;                                                                  // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value = 1 - beta2)
        const float r = __builtin_sqrtf(vv), q = r / bc2_sqrt, denom = q + eps;
        const float u = mv / denom, t4 = lr_over_bc1 * u;
        return pv - t4;                                                                // param.addcdiv_(exp_avg, denom, value = -step_size)
    };
    // ONE arithmetic instruction stream for both operand forms (whole aligned float4s / element by element): the vector and the scalar
    // branch used to carry their own copies of `one`, and the two compiled forms differed by an ulp on a few elements per tensor -- a
    // data-parallel run (gradients = views at arbitrary offsets of a flat bucket) then drifted from the single-GPU run bit by bit
    const bool vec = i0 + 4 <= n && ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(m) |
                                      reinterpret_cast<uintptr_t>(v) | reinterpret_cast<uintptr_t>(e)) & 15) == 0;
    float pv[4] = {0.f, 0.f, 0.f, 0.f}, gv[4] = {0.f, 0.f, 0.f, 0.f}, mv[4] = {0.f, 0.f, 0.f, 0.f}, vv[4] = {0.f, 0.f, 0.f, 0.f};
    float ev[4] = {0.f, 0.f, 0.f, 0.f};
    if (vec) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(p + i0), b = *reinterpret_cast<const f32x4*>(g + i0);
        const f32x4 c = *reinterpret_cast<const f32x4*>(m + i0), d = *reinterpret_cast<const f32x4*>(v + i0);
#pragma unroll
        for (int k = 0; k < 4; ++k) { pv[k] = a[k]; gv[k] = b[k]; mv[k] = c[k]; vv[k] = d[k]; }
        if constexpr (EMA) {
            const f32x4 f = *reinterpret_cast<const f32x4*>(e + i0);
#pragma unroll
            for (int k = 0; k < 4; ++k) ev[k] = f[k];
        }
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (i0 + k < n) {
                pv[k] = p[i0 + k]; gv[k] = g[i0 + k]; mv[k] = m[i0 + k]; vv[k] = v[i0 + k];
                if constexpr (EMA) ev[k] = e[i0 + k];
            }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        pv[k] = one(pv[k], gv[k], mv[k], vv[k]);
        if constexpr (EMA) ev[k] = ema_lerp_rn(ev[k], pv[k], ema_w);
    }
    if (vec) {
        *reinterpret_cast<f32x4*>(p + i0) = (f32x4){pv[0], pv[1], pv[2], pv[3]};
        *reinterpret_cast<f32x4*>(m + i0) = (f32x4){mv[0], mv[1], mv[2], mv[3]};
        *reinterpret_cast<f32x4*>(v + i0) = (f32x4){vv[0], vv[1], vv[2], vv[3]};
        if constexpr (EMA) *reinterpret_cast<f32x4*>(e + i0) = (f32x4){ev[0], ev[1], ev[2], ev[3]};
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (i0 + k < n) {
                p[i0 + k] = pv[k]; m[i0 + k] = mv[k]; v[i0 + k] = vv[k];
                if constexpr (EMA) e[i0 + k] = ev[k];
            }
    }
}

static int adam_launch(const long* jobs, const int* block_job, long total_blocks, double lr, double beta1, double beta2, double eps,
                       double weight_decay, long step, const GuardRecord* rec, const long* ema, double ema_decay, hipStream_t st) {
    // the scalars as torch forms them from Python doubles: 1 - beta, 1 - beta ** step, lr / bias_correction1, sqrt(bias_correction2) in
    // double, rounded to fp32 once (1.0f - 0.999f differs from float(0.001) by 1.3e-5); the average's weight 1 - decay likewise
    const double bc1 = 1.0 - pow(beta1, (double)step), bc2 = 1.0 - pow(beta2, (double)step);
    auto kern = ema ? (rec ? adam_step_kernel<true, true> : adam_step_kernel<false, true>)
                    : (rec ? adam_step_kernel<true, false> : adam_step_kernel<false, false>);
    hipLaunchKernelGGL(kern, dim3((unsigned)total_blocks), dim3(256), 0, st, jobs, block_job, (float)(lr / bc1), (float)(1.0 - beta1),
                       (float)beta2, (float)(1.0 - beta2), (float)eps, (float)weight_decay, (float)sqrt(bc2), rec, ema,
                       (float)(1.0 - ema_decay));
    HN_LAUNCH_CHECK();
}
extern "C" int hn_adam_step(const long* jobs, const int* block_job, long total_blocks, double lr, double beta1, double beta2, double eps,
                            double weight_decay, long step, hipStream_t st) {
    HN_CHECK_ARG(jobs && block_job && total_blocks > 0 && step >= 1 && beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0);
    return adam_launch(jobs, block_job, total_blocks, lr, beta1, beta2, eps, weight_decay, step, nullptr, nullptr, 0.0, st);
}
/* hn_adam_step that obeys the record hn_grad_guard wrote earlier on the same stream; the gradient tensors are read, never written */
extern "C" int hn_adam_step_guarded(const long* jobs, const int* block_job, long total_blocks, double lr, double beta1, double beta2, double eps,
                                    double weight_decay, long step, const void* record, hipStream_t st) {
    HN_CHECK_ARG(jobs && block_job && total_blocks > 0 && step >= 1 && beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0 && record);
    return adam_launch(jobs, block_job, total_blocks, lr, beta1, beta2, eps, weight_decay, step, (const GuardRecord*)record, nullptr, 0.0, st);
}
/* hn_adam_step (record == NULL) or hn_adam_step_guarded (record given) that also updates one moving average per job in the same launch */
extern "C" int hn_adam_step_ema(const long* jobs, const int* block_job, long total_blocks, const long* ema, double lr, double beta1,
                                double beta2, double eps, double weight_decay, long step, double ema_decay, const void* record,
                                hipStream_t st) {
    HN_CHECK_ARG(jobs && block_job && total_blocks > 0 && step >= 1 && beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0 && ema &&
                 ema_decay >= 0.0 && ema_decay < 1.0);
    return adam_launch(jobs, block_job, total_blocks, lr, beta1, beta2, eps, weight_decay, step, (const GuardRecord*)record, ema, ema_decay, st);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Global gradient norm + the step's decision, on the device (torch.nn.utils.clip_grad_norm_'s coefficient; a skip mask in place of the
// reference's host-side sys.exit() guard).  Three launches over the job tables of hn_adam_step, no atomics, no workgroup waits on another:
//   1. grad_sq_block_kernel: one fp32 value per 1024-element block.  Thread: g0*g0 + g1*g1 + g2*g2 + g3*g3 left to right, every product
//      and sum rounded (absent elements are +0, which adds exactly); block: wave_sum's fixed DPP tree, then (w0 + w1) + (w2 + w3).
//   2. grad_sq_job_kernel: one workgroup per job, in double: thread t adds the job's blocks t, t + 256, ... in ascending order, then
//      block_sum_f64's fixed tree.  3. grad_guard_final_kernel: one workgroup adds the job sums the same way and writes the record.
// The order of every addition is a function of the job table alone, so equal gradients give equal bits, run after run and whether the
// gradients are separate allocations or views at odd offsets of a bucket.
// ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void grad_sq_block_kernel(const long* jobs, const int* block_job, float* block_sq) {
    __shared__ float red[4];
    const long* jb = jobs + (long)block_job[blockIdx.x] * 6;
    const float* g = reinterpret_cast<const float*>(jb[1]);
    const long n = jb[4];
    const long i0 = (((long)blockIdx.x - jb[5]) * 256 + threadIdx.x) * 4;
    // ONE arithmetic instruction stream for both operand forms, as in adam_step_kernel
    float gv[4] = {0.f, 0.f, 0.f, 0.f};
    if (i0 + 4 <= n && (reinterpret_cast<uintptr_t>(g) & 15) == 0) {
        const f32x4 b = *reinterpret_cast<const f32x4*>(g + i0);
#pragma unroll
        for (int k = 0; k < 4; ++k) gv[k] = b[k];
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (i0 + k < n) gv[k] = g[i0 + k];
    }
    float s = __fmul_rn(gv[0], gv[0]);
#pragma unroll
    for (int k = 1; k < 4; ++k) s = __fadd_rn(s, __fmul_rn(gv[k], gv[k]));
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) block_sq[blockIdx.x] = __fadd_rn(__fadd_rn(red[0], red[1]), __fadd_rn(red[2], red[3]));
}

// sum of 256 doubles in a fixed tree (xor butterflies inside each wave, then the four waves through LDS); thread 0's value is used
__device__ __forceinline__ double block_sum_f64(double v, double* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = __dadd_rn(v, __shfl_xor(v, o));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return __dadd_rn(__dadd_rn(red[0], red[1]), __dadd_rn(red[2], red[3]));
}

__global__ __launch_bounds__(256) void grad_sq_job_kernel(const long* jobs, const float* block_sq, double* job_sum, double* job_sq) {
    __shared__ double red[4];
    const long* jb = jobs + (long)blockIdx.x * 6;
    const long nb = (jb[4] + 1023) / 1024;
    const float* bs = block_sq + jb[5];
    double s = 0.0;
    for (long b = threadIdx.x; b < nb; b += 256) s = __dadd_rn(s, (double)bs[b]);
    s = block_sum_f64(s, red);
    if (threadIdx.x == 0) {
        job_sum[blockIdx.x] = s;
        if (job_sq) job_sq[blockIdx.x] = s;
    }
}

struct GuardArgs {
    const double* job_sum;
    long n_jobs;
    float max_norm;
    int flags, n_losses, n_words;
    const float* losses[8];
    const int* words[4];
    GuardRecord* rec;
};
__global__ __launch_bounds__(256) void grad_guard_final_kernel(GuardArgs a) {
    __shared__ double red[4];
    double s = 0.0;
    for (long j = threadIdx.x; j < a.n_jobs; j += 256) s = __dadd_rn(s, a.job_sum[j]);
    s = block_sum_f64(s, red);
    if (threadIdx.x != 0) return;
    const float norm = (float)sqrt(s);
    float coef = 1.0f;
    if (a.max_norm > 0.f) {
        // clip_grad_norm_: clamp(max_norm / (total_norm + 1e-6), max = 1.0); a NaN stays a NaN, as torch.clamp leaves it
        const float c = __fdiv_rn(a.max_norm, __fadd_rn(norm, 1e-6f));
        coef = c < 1.0f || c != c ? c : 1.0f;
    }
    int skip = 0;
    if (a.flags & 1) {
        if (!(s <= (double)__FLT_MAX__)) skip |= 1;                    // NaN, inf, or past fp32's range (torch's fp32 norm is inf there)
        for (int i = 0; i < a.n_losses; ++i)
            if (!(fabsf(a.losses[i][0]) <= __FLT_MAX__)) skip |= 2;
    }
    for (int i = 0; i < a.n_words; ++i)
        if (a.words[i][0] != 0) skip |= 4;
    GuardRecord* r = a.rec;
    r->norm = norm;
    r->coef = coef;
    r->skip = skip;
    r->steps += 1;
    if (skip) { r->skipped += 1; r->skipped_consecutive += 1; }
    else r->skipped_consecutive = 0;
}

static inline long align16(long x) { return (x + 15) & ~15L; }
extern "C" long hn_grad_guard_ws_bytes(long total_blocks, long n_jobs) {
    if (total_blocks < 1 || total_blocks > 0x7fffffffL || n_jobs < 1 || n_jobs > total_blocks) return -1;
    return align16(total_blocks * 4) + align16(n_jobs * 8);
}
extern "C" int hn_grad_guard(const long* jobs, const int* block_job, long total_blocks, long n_jobs, double max_norm, int flags,
                             const void* const* losses, int n_losses, const void* const* words, int n_words, void* ws, long ws_bytes,
                             double* job_sq, void* record, hipStream_t st) {
    const long need = hn_grad_guard_ws_bytes(total_blocks, n_jobs);
    HN_CHECK_ARG(jobs && block_job && need > 0 && ws && ws_bytes >= need && (reinterpret_cast<uintptr_t>(ws) & 15) == 0 && record &&
                 (reinterpret_cast<uintptr_t>(record) & 3) == 0 && max_norm == max_norm && n_losses >= 0 && n_losses <= 8 && n_words >= 0 &&
                 n_words <= 4 && (n_losses == 0 || losses) && (n_words == 0 || words));
    GuardArgs a = {};
    for (int i = 0; i < n_losses; ++i) { HN_CHECK_ARG(losses[i]); a.losses[i] = (const float*)losses[i]; }
    for (int i = 0; i < n_words; ++i) { HN_CHECK_ARG(words[i]); a.words[i] = (const int*)words[i]; }
    float* block_sq = (float*)ws;
    double* job_sum = (double*)((char*)ws + align16(total_blocks * 4));
    a.job_sum = job_sum; a.n_jobs = n_jobs; a.max_norm = (float)max_norm; a.flags = flags; a.n_losses = n_losses; a.n_words = n_words;
    a.rec = (GuardRecord*)record;
    hipLaunchKernelGGL(grad_sq_block_kernel, dim3((unsigned)total_blocks), dim3(256), 0, st, jobs, block_job, block_sq);
    hipLaunchKernelGGL(grad_sq_job_kernel, dim3((unsigned)n_jobs), dim3(256), 0, st, jobs, (const float*)block_sq, job_sum, job_sq);
    hipLaunchKernelGGL(grad_guard_final_kernel, dim3(1), dim3(256), 0, st, a);
    HN_LAUNCH_CHECK();
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Many fp32 tensors copied (or rounded to bf16) in ONE launch: the gather of a gradient bucket before its all-reduce and the scatter of
// a reduced-precision payload back to fp32 (torch._foreach_copy_ issues one launch per ~50 tensors: 14 launches, 0.5 ms per step for the
// 693 gradients).  jobs (device): n x {src, dst, numel, first_block}; block = 256 threads x 4 elements; kind: 0 f32 -> f32, 1 f32 -> bf16,
// 2 bf16 -> f32.
// ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void copy_many_kernel(const long* jobs, const int* block_job, int kind) {
    const long* jb = jobs + (long)block_job[blockIdx.x] * 4;
    const long n = jb[2];
    const long i0 = (((long)blockIdx.x - jb[3]) * 256 + threadIdx.x) * 4;
    if (i0 >= n) return;
    const int cnt = n - i0 < 4 ? (int)(n - i0) : 4;
    if (kind == 0) {
        const float* s = reinterpret_cast<const float*>(jb[0]) + i0;
        float* d = reinterpret_cast<float*>(jb[1]) + i0;
        if (cnt == 4 && ((reinterpret_cast<uintptr_t>(s) | reinterpret_cast<uintptr_t>(d)) & 15) == 0) *reinterpret_cast<f32x4*>(d) = *reinterpret_cast<const f32x4*>(s);
        else for (int k = 0; k < cnt; ++k) d[k] = s[k];
    } else if (kind == 1) {
        const float* s = reinterpret_cast<const float*>(jb[0]) + i0;
        bf16* d = reinterpret_cast<bf16*>(jb[1]) + i0;
        for (int k = 0; k < cnt; ++k) d[k] = f2bf(s[k]);
    } else {
        const bf16* s = reinterpret_cast<const bf16*>(jb[0]) + i0;
        float* d = reinterpret_cast<float*>(jb[1]) + i0;
        for (int k = 0; k < cnt; ++k) d[k] = bf2f(s[k]);
    }
}

extern "C" int hn_copy_many(const long* jobs, const int* block_job, long total_blocks, int kind, hipStream_t st) {
    HN_CHECK_ARG(jobs && block_job && total_blocks > 0 && kind >= 0 && kind <= 2);
    hipLaunchKernelGGL(copy_many_kernel, dim3((unsigned)total_blocks), dim3(256), 0, st, jobs, block_job, kind);
    HN_LAUNCH_CHECK();
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Many pairs of fp32 tensors exchanged element by element in ONE launch (optim.Adam.swap_ema: the averaged weights in, the live ones out,
// through the same addresses -- a captured step, the optimizer's tables and the eval-mode caches keep their pointers).  hn_copy_many's
// tables: jobs (device) n x {a, b, numel, first_block}.  32-bit words are moved, never floats: NaN payloads and -0 survive.  a and b of a
// job do not overlap; every thread reads its own elements of both before it writes either, and no thread touches another's.
// ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void swap_many_kernel(const long* jobs, const int* block_job) {
    const long* jb = jobs + (long)block_job[blockIdx.x] * 4;
    const long n = jb[2];
    const long i0 = (((long)blockIdx.x - jb[3]) * 256 + threadIdx.x) * 4;
    if (i0 >= n) return;
    const int cnt = n - i0 < 4 ? (int)(n - i0) : 4;
    unsigned* a = reinterpret_cast<unsigned*>(jb[0]) + i0;
    unsigned* b = reinterpret_cast<unsigned*>(jb[1]) + i0;
    if (cnt == 4 && ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 15) == 0) {
        const uint4 x = *reinterpret_cast<const uint4*>(a), y = *reinterpret_cast<const uint4*>(b);
        *reinterpret_cast<uint4*>(a) = y;
        *reinterpret_cast<uint4*>(b) = x;
    } else {
        for (int k = 0; k < cnt; ++k) {
            const unsigned x = a[k], y = b[k];
            a[k] = y;
            b[k] = x;
        }
    }
}

extern "C" int hn_swap_many(const long* jobs, const int* block_job, long total_blocks, hipStream_t st) {
    HN_CHECK_ARG(jobs && block_job && total_blocks > 0);
    hipLaunchKernelGGL(swap_many_kernel, dim3((unsigned)total_blocks), dim3(256), 0, st, jobs, block_job);
    HN_LAUNCH_CHECK();
}
