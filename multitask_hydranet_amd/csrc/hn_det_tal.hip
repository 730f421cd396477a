// Task-aligned anchor assignment (TAL; Feng et al., TOOD, 2021; detection.assigner = tal).  Per image, anchors (y1, x1, y2, x2),
// annotations (x1, y1, x2, y2, class; class -1 = padding), regression [A][4] and post-sigmoid classification [A][K], both read as constants:
//
//   u(a, j)     the iou of det_iou_box (hn_det_common.h) for anchor a's regression against box j: the deploy decode with the log(1000/16)
//               clip on dh and dw, target sides clamped to at least 1, eps 1e-7 -- the number the regression loss, pos_iou and the quality
//               targets are made of
//   s(a, j)     classification[a][class_j], unclamped; 0 for a class id outside 0 .. K - 1
//   t(a, j)     s ((u u) (u u)) (u u) in fp32: the alignment metric s^alpha u^beta with alpha = 1, beta = 6
//   eligible    the anchor's centre lies inside the raw annotation by more than 0.01 px (ATSS's rule:
//               min(acx - x1, acy - y1, x2 - acx, y2 - acy) > 0.01) and t > 0 (a NaN or zero metric never is; a NaN anywhere in
//               the anchor's regression makes its t NaN)
//   candidates  of box j: its topk eligible anchors with the largest (t, then lower anchor index); all of them when fewer are eligible
//   conflicts   a candidate of several boxes goes to the largest u, ties to the lowest annotation index
//   otherwise   -1 (background); an image without valid annotations is all -1; there is no ignore zone (-2 never appears)
//   target      with tmax, umax the maxima of t, u over the anchors finally assigned to box j: (t / tmax) umax for an assigned anchor (both
//               operations individually rounded), 0 for every other anchor
//
// Three launches, none waits on another workgroup, no float atomics, nothing whose result depends on an order:
//   select     one workgroup per (box, image) walks the A anchors; the inside test comes first (most anchors fail it), only then the decode,
//              the IoU and the one score load.  The 64-bit key of an eligible pair is (~bits of t) << 32 | anchor index (t > 0: the bit
//              pattern orders like the value), so the topk-th SMALLEST key is wanted.  A first walk takes the maximum t of each of 256
//              strided shares of the anchors (1024 threads, four to a share); the topk-th largest of these maxima bounds the topk-th
//              largest t from below (they are topk different anchors), and a second walk puts the keys with t at or above that bound (a few dozen) into an LDS list, on which
//              a radix select (11-bit digits, LDS histogram) runs.  When the list overflows (masses of equal metrics, or topk above the
//              256 shares with thousands of eligible anchors) the same select runs on keys recomputed from global memory.
//   assign     one thread per (image, anchor): the anchor is a candidate of box j exactly when its own key is at most the stored key of j;
//              the loop over the boxes applies the conflict rule and writes assign, the pair's t and, by integer atomic max on the bit
//              patterns of the non-negative floats (order-free), the per-box maxima
//   normalise  one thread per (image, anchor): t <- (t / tmax) umax
// The metric of a pair is one function that is NOT inlined (tal_metric), so the select and the assign launch get its bits from the same
// instructions whatever the compiler contracts inside the box function.
#include "hn_common.h"
#include "hn_det_common.h"

#define HN_TAL_THREADS 1024                                            // select workgroup: 16 waves on one CU hide the walk's load and exp latency
#define HN_TAL_SHARES 256                                              // strided shares of the prefilter (thread t is in share t % 256)
#define HN_TAL_BINS 2048
#define HN_TAL_LIST 2048                                               // prefiltered keys of one box held in LDS; the largest topk

struct TalTU { float t, u; };

__device__ __noinline__ TalTU tal_metric(f32x4 anc, f32x4 reg, float bx1, float by1, float bx2, float by2, float s) {
    const float a[4] = {anc[0], anc[1], anc[2], anc[3]}, r[4] = {reg[0], reg[1], reg[2], reg[3]}, b[4] = {bx1, by1, bx2, by2};
    float loss, u;
    det_iou_box<false>(r, a, b, 1, loss, u, nullptr);
    const float u2 = u * u;
    TalTU m;
    m.t = (s * (u2 * u2)) * u2;
    m.u = u;
    // (the box function's fminf / fmaxf drop a NaN operand, so a NaN regression would come out as a finite u: it makes the metric NaN here)
    if (reg[0] != reg[0] || reg[1] != reg[1] || reg[2] != reg[2] || reg[3] != reg[3]) m.t = __builtin_nanf("");
    return m;
}

// the class of an annotation as an index into the scores, -1 when it matches none
__device__ __forceinline__ int tal_class(float c, int K) { return c >= 0.f && c < (float)K ? (int)c : -1; }

__device__ __forceinline__ f32x4 tal_anchor(const float* anchors, int a) { return *reinterpret_cast<const f32x4*>(anchors + (long)a * 4); }

// the pair (anchor a = anc, box b = (x1, y1, x2, y2) with class index cid >= 0) of image n: false unless eligible, else its metric
__device__ __forceinline__ bool tal_pair(f32x4 anc, const float* reg_n, const float* cls_n, int K, int a, f32x4 b, int cid, TalTU& m) {
    const float acy = (anc[0] + anc[2]) * 0.5f, acx = (anc[1] + anc[3]) * 0.5f;
    const float side = fminf(fminf(acx - b[0], acy - b[1]), fminf(b[2] - acx, b[3] - acy));
    if (!(side > 0.01f)) return false;
    const f32x4 reg = *reinterpret_cast<const f32x4*>(reg_n + (long)a * 4);
    m = tal_metric(anc, reg, b[0], b[1], b[2], b[3], cls_n[(long)a * K + cid]);
    return m.t > 0.f;
}
// smaller key = larger t, then lower index
__device__ __forceinline__ unsigned long long tal_key(float t, int idx) {
    return ((unsigned long long)(~__float_as_uint(t)) << 32) | (unsigned int)idx;
}
__device__ __forceinline__ float tal_target(float t, float tmax, float umax) {
#pragma clang fp contract(off)
    const float q = t / tmax;
    return q * umax;
}

// ws layout: kth u64 [N][Mx] | bmax u32 [N][Mx][2] (bits of tmax, umax)
__global__ __launch_bounds__(HN_TAL_THREADS) void tal_select_kernel(const float* anchors, const float* reg, const float* cls, const float* ann, int A,
                                                                    int K, int Mx, int topk, unsigned long long* kth, unsigned int* bmax) {
    __shared__ unsigned int hist[HN_TAL_BINS];
    __shared__ unsigned long long list[HN_TAL_LIST];
    __shared__ unsigned int maxs[HN_TAL_SHARES];                       // bits of the maximum t over the eligible anchors of each share
    __shared__ unsigned int wsum[4];
    __shared__ unsigned int s_bin, s_rank, s_cnt, s_bound;
    const int j = blockIdx.x, n = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long pair = (long)n * Mx + j;
    if (tid == 0) { bmax[pair * 2] = 0u; bmax[pair * 2 + 1] = 0u; }     // (the assign launch takes maxima into them)
    const float* bp = ann + pair * 5;
    if (bp[4] == -1.f) return;                                         // padding row: nothing of it is ever read (uniform exit)
    const int cid = tal_class(bp[4], K);
    const f32x4 b = {bp[0], bp[1], bp[2], bp[3]};
    if (cid < 0) {                                                     // s = 0 throughout: nothing is eligible (uniform exit)
        if (tid == 0) kth[pair] = 0ull;
        return;
    }
    const float* reg_n = reg + (long)n * A * 4;
    const float* cls_n = cls + (long)n * A * K;
    if (tid == 0) { s_bin = 0; s_rank = 1; s_cnt = 0; s_bound = 0u; }

    // the bound: the topk-th largest of the shares' maxima (ties ranked by share); 0 = every eligible anchor when topk exceeds the
    // shares or fewer than topk shares hold an eligible anchor.  Both walks load four anchors ahead of the (opaque) metric calls.
    if (tid < HN_TAL_SHARES) maxs[tid] = 0u;
    __syncthreads();
    unsigned int mine = 0u;
    for (int i0 = tid; i0 < A; i0 += 4 * HN_TAL_THREADS) {
        f32x4 an[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) an[q] = tal_anchor(anchors, i0 + q * HN_TAL_THREADS < A ? i0 + q * HN_TAL_THREADS : 0);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int i = i0 + q * HN_TAL_THREADS;
            TalTU m;
            if (i < A && tal_pair(an[q], reg_n, cls_n, K, i, b, cid, m)) mine = max(mine, __float_as_uint(m.t));
        }
    }
    if (mine) atomicMax(&maxs[tid & (HN_TAL_SHARES - 1)], mine);
    __syncthreads();
    if (topk <= HN_TAL_SHARES && tid < HN_TAL_SHARES) {
        const unsigned int own = maxs[tid];
        int r = 0;
        for (int q = 0; q < HN_TAL_SHARES; ++q) {
            const unsigned int o = maxs[q];
            r += (o > own || (o == own && q < tid)) ? 1 : 0;
        }
        if (r == topk - 1) s_bound = own;
    }
    __syncthreads();
    const unsigned int bound = s_bound;
    for (int i0 = tid; i0 < A; i0 += 4 * HN_TAL_THREADS) {
        f32x4 an[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) an[q] = tal_anchor(anchors, i0 + q * HN_TAL_THREADS < A ? i0 + q * HN_TAL_THREADS : 0);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int i = i0 + q * HN_TAL_THREADS;
            TalTU m;
            if (i < A && tal_pair(an[q], reg_n, cls_n, K, i, b, cid, m) && __float_as_uint(m.t) >= bound) {
                const unsigned int p = atomicAdd(&s_cnt, 1u);
                if (p < HN_TAL_LIST) list[p] = tal_key(m.t, i);
            }
        }
    }
    __syncthreads();
    const int nlist = (int)s_cnt;
    __syncthreads();
    if (nlist < topk) {                                                // fewer than topk eligible (the bound was 0): all of them (uniform exit)
        if (tid == 0) kth[pair] = ~0ull;
        return;
    }
    const bool in_lds = nlist <= HN_TAL_LIST;                           // uniform
    const int nsrc = in_lds ? nlist : A;

    // digits, most significant first: the 31 value bits of ~t (bit 63 is set in every key: t > 0) as 11 + 11 + 9, then the index bits that
    // A - 1 can have, 11 at a time.  The index digits are skipped when the t digits end with every remaining tie taken.
    int nb = 0;
    while (nb < 31 && (A - 1) >> nb) ++nb;
    unsigned long long prefix = 1ull << 63;
    unsigned int rank = (unsigned int)topk;                            // 1-based rank inside the still-ambiguous set
    bool all_ties = false;
    for (int seg = 0; seg < 2 && !all_ties; ++seg) {
        const int base = seg == 0 ? 32 : 0;
        for (int hi = seg == 0 ? 31 : nb; hi > 0; hi -= 11) {
            const int lo = hi > 11 ? hi - 11 : 0, width = hi - lo, shift = base + lo;
            for (int i = tid; i < HN_TAL_BINS; i += HN_TAL_THREADS) hist[i] = 0;
            __syncthreads();
            for (int i = tid; i < nsrc; i += HN_TAL_THREADS) {
                unsigned long long key;
                if (in_lds) {
                    key = list[i];
                } else {
                    TalTU m;
                    if (!tal_pair(tal_anchor(anchors, i), reg_n, cls_n, K, i, b, cid, m)) continue;
                    key = tal_key(m.t, i);
                }
                if (((key ^ prefix) >> (shift + width)) == 0) atomicAdd(&hist[(unsigned int)(key >> shift) & ((1u << width) - 1u)], 1u);
            }
            __syncthreads();
            // thread t < 256 (the first four waves, whole) owns bins 8t .. 8t + 7: an inclusive scan of the per-thread sums inside each
            // wave and across the four, then the one thread whose range holds the rank walks its eight bins
            unsigned int own = 0, incl = 0;
            if (tid < 256) {
#pragma unroll
                for (int q = 0; q < 8; ++q) own += hist[tid * 8 + q];
                incl = own;
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) {
                    const unsigned int t = __shfl_up(incl, d);
                    if (lane >= d) incl += t;
                }
                if (lane == 63) wsum[wave] = incl;
            }
            __syncthreads();
            if (tid < 256) {
                for (int w2 = 0; w2 < wave; ++w2) incl += wsum[w2];
                unsigned int excl = incl - own;
                if (excl < rank && rank <= incl) {
                    for (int q = 0; q < 8; ++q) {
                        const unsigned int c = hist[tid * 8 + q];
                        if (rank <= excl + c) { s_bin = (unsigned int)(tid * 8 + q); s_rank = rank - excl; s_cnt = c; break; }
                        excl += c;
                    }
                }
            }
            __syncthreads();
            prefix |= (unsigned long long)s_bin << shift;
            rank = s_rank;
            if (seg == 0 && lo == 0 && s_cnt == rank) all_ties = true;
            __syncthreads();                                           // (s_* and hist are rewritten by the next digit)
        }
    }
    if (all_ties) prefix |= 0xffffffffull;
    if (tid == 0) kth[pair] = prefix;
}

__global__ __launch_bounds__(256) void tal_assign_kernel(const float* anchors, const float* reg, const float* cls, const float* ann, int A, int K,
                                                         int Mx, const unsigned long long* kth, unsigned int* bmax, short* assign, float* target) {
    const int n = blockIdx.y;
    const int a = blockIdx.x * 256 + threadIdx.x;
    if (a >= A) return;
    const float* reg_n = reg + (long)n * A * 4;
    const float* cls_n = cls + (long)n * A * K;
    const f32x4 anc = tal_anchor(anchors, a);
    float best = -1.f, bt = 0.f;
    int arg = -1;
    for (int j = 0; j < Mx; ++j) {
        const float* bp = ann + ((long)n * Mx + j) * 5;
        if (bp[4] == -1.f) continue;
        const int cid = tal_class(bp[4], K);
        if (cid < 0) continue;
        TalTU m;
        if (!tal_pair(anc, reg_n, cls_n, K, a, f32x4{bp[0], bp[1], bp[2], bp[3]}, cid, m)) continue;
        if (tal_key(m.t, a) > kth[(long)n * Mx + j]) continue;
        if (m.u > best) { best = m.u; arg = j; bt = m.t; }             // the lowest annotation index wins a tie
    }
    assign[(long)n * A + a] = (short)arg;
    target[(long)n * A + a] = bt;
    if (arg >= 0) {                                                    // (t > 0 and u > 0: the bit patterns order like the values)
        atomicMax(&bmax[((long)n * Mx + arg) * 2], __float_as_uint(bt));
        atomicMax(&bmax[((long)n * Mx + arg) * 2 + 1], __float_as_uint(best));
    }
}

__global__ __launch_bounds__(256) void tal_normalise_kernel(int A, int Mx, const unsigned int* bmax, const short* assign, float* target) {
    const int n = blockIdx.y;
    const int a = blockIdx.x * 256 + threadIdx.x;
    if (a >= A) return;
    const int as = assign[(long)n * A + a];
    if (as < 0) return;                                                // (its target is the 0 the assign launch wrote)
    const unsigned int* bm = bmax + ((long)n * Mx + as) * 2;
    target[(long)n * A + a] = tal_target(target[(long)n * A + a], __uint_as_float(bm[0]), __uint_as_float(bm[1]));
}

static bool tal_args_ok(int N, int A, int Mx, int topk) {
    return N > 0 && N <= 65535 && A > 0 && Mx > 0 && Mx <= 32767 && topk >= 1 && topk <= HN_TAL_LIST;      // grid y, int16 assign, the LDS list
}
static long tal_kth_bytes(int N, int Mx) { return (((long)N * Mx * 8) + 255) / 256 * 256; }

// workspace bytes of hn_det_tal_assign; -1 for arguments hn_det_tal_assign would reject
extern "C" long hn_det_tal_ws_bytes(int N, int A, int Mx, int topk) {
    if (!tal_args_ok(N, A, Mx, topk)) return -1;
    return tal_kth_bytes(N, Mx) + (long)N * Mx * 8;
}

// anchors fp32 [A][4], regression fp32 [N][A][4], classification fp32 [N][A][K] (post-sigmoid), ann fp32 [N][Mx][5], ws: hn_det_tal_ws_bytes
// bytes; writes assign int16 [N][A] (>= 0 matched annotation, -1 background) and target fp32 [N][A] (the aligned classification target of an
// assigned anchor, else 0)
extern "C" int hn_det_tal_assign(const float* anchors, const float* regression, const float* classification, const float* ann, int N, int A, int K,
                                 int Mx, int topk, void* ws, void* assign, float* target, hipStream_t st) {
    HN_CHECK_ARG((((uintptr_t)anchors | (uintptr_t)regression) & 15) == 0);      // an anchor and its regression are one 16-byte load each
    HN_CHECK_ARG(anchors && regression && classification && ann && ws && assign && target);
    HN_CHECK_ARG(tal_args_ok(N, A, Mx, topk) && K > 0 && K <= HN_DET_MAXK);
    unsigned long long* kth = (unsigned long long*)ws;
    unsigned int* bmax = (unsigned int*)((char*)ws + tal_kth_bytes(N, Mx));
    hipLaunchKernelGGL(tal_select_kernel, dim3(Mx, N), dim3(HN_TAL_THREADS), 0, st, anchors, regression, classification, ann, A, K, Mx, topk, kth,
                       bmax);
    hipLaunchKernelGGL(tal_assign_kernel, dim3((A + 255) / 256, N), dim3(256), 0, st, anchors, regression, classification, ann, A, K, Mx,
                       (const unsigned long long*)kth, bmax, (short*)assign, target);
    hipLaunchKernelGGL(tal_normalise_kernel, dim3((A + 255) / 256, N), dim3(256), 0, st, A, Mx, (const unsigned int*)bmax, (const short*)assign,
                       target);
    HN_LAUNCH_CHECK();
}
