// ATSS anchor assignment (adaptive training sample selection; detection.assigner = atss).  Per image, anchors (y1, x1, y2, x2),
// annotations (x1, y1, x2, y2, class; class -1 = padding):
//
//   centres     acy = (y1 + y2) 0.5, acx = (x1 + x2) 0.5 of an anchor; gcx = (x1 + x2) 0.5, gcy = (y1 + y2) 0.5 of a box
//   distance    d2 = dx dx + dy dy, every operation an individually rounded fp32 operation (atss_d2 below: no contraction), so a numpy
//               float32 restatement reproduces the keys bit for bit
//   candidates  on level l (a contiguous anchor range of A_l anchors) the k_l = min(topk anchors_per_location, A_l) anchors with the
//               smallest (d2, anchor index); ties in d2 go to the lower index
//   threshold   thr = mean + std of the IoUs (det_assign's formula) of a box's candidates over all levels; std unbiased (n - 1), two
//               passes, 0 when n < 2
//   positive    a candidate with iou >= thr whose centre is inside the box by more than 0.01 px:
//               min(acx - x1, acy - y1, x2 - acx, y2 - acy) > 0.01
//   conflicts   an anchor positive for several boxes goes to the largest IoU, ties to the lowest annotation index
//   otherwise   -1 (background); an image without valid annotations is all -1; there is no ignore zone (-2 never appears)
//
// Three launches, none waits on another workgroup, no float atomics, fixed summation orders:
//   select   one workgroup per (level, box, image): radix select (11-bit digits, LDS histogram) of the k_l-th smallest 64-bit key
//            (d2 bits << 32) | index-in-level over the level's anchors (d2 >= 0: the bit pattern orders like the value), after a
//            prefilter that leaves a few hundred keys in LDS; then the candidates' IoUs are gathered and written in index order
//   thr      one workgroup per (box, image): mean, second pass, thr[N][Mx]
//   assign   one thread per (image, anchor): an anchor is a candidate of box j exactly when its own key is at most the stored key of
//            (j, its level); a loop over the boxes of the shape of det_assign's decides the rest
// The loss forwards then read assign (hn_det_loss_fwd_assigned / hn_det_loss_iou_fwd_assigned); the backwards always did.
#include "hn_common.h"
#include "hn_det_common.h"

#define HN_ATSS_MAX_LEVELS 8
#define HN_ATSS_MAXK 1024                                              // candidates per (box, level): two LDS lists of this length
#define HN_ATSS_BINS 2048
#define HN_ATSS_THREADS 256                                            // select workgroup (a multiple of 256; 1024 measured slower)
#define HN_ATSS_LIST 2048                                              // prefiltered keys of one (box, level) held in LDS

struct AtssLevels {
    int n;
    int off[HN_ATSS_MAX_LEVELS + 1];                                   // level l = anchors [off[l], off[l + 1])
    int k[HN_ATSS_MAX_LEVELS];                                         // candidates per box on level l
    int koff[HN_ATSS_MAX_LEVELS + 1];                                  // prefix sums of k
};

// squared centre distance; three products / sums and the two centre halvings, each rounded on its own
__device__ __forceinline__ float atss_d2(const float* anc, float gcx, float gcy) {
#pragma clang fp contract(off)
    const float sy = anc[0] + anc[2], sx = anc[1] + anc[3];
    const float acy = sy * 0.5f, acx = sx * 0.5f;
    const float dx = acx - gcx, dy = acy - gcy;
    const float xx = dx * dx, yy = dy * dy;
    return xx + yy;
}
__device__ __forceinline__ void atss_box_centre(const float* b, float& gcx, float& gcy) {
#pragma clang fp contract(off)
    const float sx = b[0] + b[2], sy = b[1] + b[3];
    gcx = sx * 0.5f;
    gcy = sy * 0.5f;
}
__device__ __forceinline__ unsigned long long atss_key(float d2, int idx) {
    return ((unsigned long long)__float_as_uint(d2) << 32) | (unsigned int)idx;
}
// det_assign's IoU (union clamped at 1e-8), without contraction so that the select and the assign kernel get the same bits
__device__ __forceinline__ float atss_iou(const float* anc, const float* b) {
#pragma clang fp contract(off)
    const float ay1 = anc[0], ax1 = anc[1], ay2 = anc[2], ax2 = anc[3];
    const float aarea = (ay2 - ay1) * (ax2 - ax1);
    const float area = (b[2] - b[0]) * (b[3] - b[1]);
    float iw = fminf(ax2, b[2]) - fmaxf(ax1, b[0]);
    float ih = fminf(ay2, b[3]) - fmaxf(ay1, b[1]);
    iw = fmaxf(iw, 0.f);
    ih = fmaxf(ih, 0.f);
    const float inter = iw * ih;
    float ua = aarea + area - inter;
    ua = fmaxf(ua, 1e-8f);
    return inter / ua;
}

// sum over the block's 256 threads in a fixed order (wave sums, then the four waves in order); every thread gets the total
__device__ __forceinline__ float atss_block_sum(float v, float* red /* [4] LDS */) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

// one anchor (y1, x1, y2, x2) as one 16-byte load
__device__ __forceinline__ float atss_d2_at(const float* anc, int i, float gcx, float gcy) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(anc + (long)i * 4);
    const float a[4] = {v[0], v[1], v[2], v[3]};
    return atss_d2(a, gcx, gcy);
}

// ws layout: kth u64 [N][Mx][L] | cand fp32 [N][Mx][ktot]
//
// A level has up to 73 728 anchors and a box wants its 81 nearest, so the select first shrinks the problem (two walks over the level,
// no histogram): the minimum d2 of each of 256 strided shares of the level is taken; the k_l-th smallest of the 256 minima bounds the k_l-th
// smallest d2 of the level from above (they are k_l different anchors), and the keys with d2 <= that bound (a few hundred) go to an
// LDS list on which the radix select and the gather then run.  A level whose list would overflow (masses of equal distances) or whose
// k_l exceeds the 256 minima runs the same select on the anchors in global memory instead.
__global__ __launch_bounds__(HN_ATSS_THREADS) void atss_select_kernel(const float* anchors, const float* ann, int Mx, AtssLevels L, unsigned long long* kth,
                                                          float* cand) {
    __shared__ unsigned int hist[HN_ATSS_BINS];
    __shared__ unsigned long long list[HN_ATSS_LIST];
    __shared__ unsigned int mins[256];                                 // bits of the minimum d2 over the anchors i with i % 256 == g
    __shared__ unsigned int wsum[4];
    __shared__ unsigned int s_bin, s_rank, s_cnt, s_bound;
    __shared__ int c_idx[HN_ATSS_MAXK];
    __shared__ float c_iou[HN_ATSS_MAXK];
    const int l = blockIdx.x, j = blockIdx.y, n = blockIdx.z;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* b = ann + ((long)n * Mx + j) * 5;
    if (b[4] == -1.f) return;                                          // padding row: nothing of it is ever read (uniform exit)
    const int a0 = L.off[l], Al = L.off[l + 1] - a0, kl = L.k[l];
    const float* anc = anchors + (long)a0 * 4;
    float gcx, gcy;
    atss_box_centre(b, gcx, gcy);
    // (a NaN box matches nothing: the select then ends on these values, in bounds)
    if (tid == 0) { s_bin = 0; s_rank = 1; s_cnt = 0; s_bound = 0x7f800000u; }

    // the bound: the k_l-th smallest of the per-thread minima (ties ranked by thread), +inf when there are more candidates than threads
    if (tid < 256) mins[tid] = 0x7f800000u;
    __syncthreads();
    float mn = __builtin_inff();
#pragma unroll 4
    for (int i = tid; i < Al; i += HN_ATSS_THREADS) mn = fminf(mn, atss_d2_at(anc, i, gcx, gcy));
    atomicMin(&mins[tid & 255], __float_as_uint(mn));                  // (mn >= 0 and never NaN: the bits order like the value)
    __syncthreads();
    if (kl <= 256 && tid < 256) {
        const unsigned int mine = mins[tid];
        int r = 0;
        for (int q = 0; q < 256; ++q) {
            const unsigned int o = mins[q];
            r += (o < mine || (o == mine && q < tid)) ? 1 : 0;
        }
        if (r == kl - 1) s_bound = mine;
    }
    __syncthreads();
    const unsigned int bound = s_bound;
#pragma unroll 4
    for (int i = tid; i < Al; i += HN_ATSS_THREADS) {
        const float d2 = atss_d2_at(anc, i, gcx, gcy);
        if (__float_as_uint(d2) <= bound) {                            // (d2 >= 0: the bits order like the value; a NaN is above +inf)
            const unsigned int p = atomicAdd(&s_cnt, 1u);
            if (p < HN_ATSS_LIST) list[p] = atss_key(d2, i);
        }
    }
    __syncthreads();
    const int nlist = (int)s_cnt;
    const bool in_lds = nlist <= HN_ATSS_LIST;                          // uniform
    const int nsrc = in_lds ? nlist : Al;
    __syncthreads();

    // digits, most significant first: d2's 31 value bits as 11 + 11 + 9, then the index bits that A_l - 1 can have, 11 at a time.  The
    // index digits are skipped when the d2 digits end with every remaining tie taken (the common case: the anchors of one location tie).
    int nb = 0;
    while (nb < 31 && (Al - 1) >> nb) ++nb;
    unsigned long long prefix = 0;
    unsigned int rank = (unsigned int)kl;                              // 1-based rank inside the still-ambiguous set
    bool all_ties = false;
    for (int seg = 0; seg < 2 && !all_ties; ++seg) {
        const int base = seg == 0 ? 32 : 0;
        for (int hi = seg == 0 ? 31 : nb; hi > 0; hi -= 11) {
            const int lo = hi > 11 ? hi - 11 : 0, width = hi - lo, shift = base + lo;
            for (int i = tid; i < HN_ATSS_BINS; i += HN_ATSS_THREADS) hist[i] = 0;
            __syncthreads();
            for (int i = tid; i < nsrc; i += HN_ATSS_THREADS) {
                const unsigned long long key = in_lds ? list[i] : atss_key(atss_d2_at(anc, i, gcx, gcy), i);
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
    if (tid == 0) kth[((long)n * Mx + j) * L.n + l] = prefix;

    // the candidates (exactly k_l keys are <= prefix), gathered in arrival order and written in index order
    if (tid == 0) s_cnt = 0;
    __syncthreads();
    for (int i = tid; i < nsrc; i += HN_ATSS_THREADS) {
        const unsigned long long key = in_lds ? list[i] : atss_key(atss_d2_at(anc, i, gcx, gcy), i);
        if (key <= prefix) {
            const int idx = (int)(unsigned int)key;                    // (< A_l: it came from this level's walk)
            const unsigned int p = atomicAdd(&s_cnt, 1u);
            if (p < HN_ATSS_MAXK) { c_idx[p] = idx; c_iou[p] = atss_iou(anc + (long)idx * 4, b); }
        }
    }
    __syncthreads();
    float* out = cand + ((long)n * Mx + j) * L.koff[L.n] + L.koff[l];
    for (int i = tid; i < kl; i += HN_ATSS_THREADS) {
        const int me = c_idx[i];
        int r = 0;
        for (int q = 0; q < kl; ++q) r += c_idx[q] < me ? 1 : 0;
        out[r] = c_iou[i];
    }
}

__global__ __launch_bounds__(256) void atss_thr_kernel(const float* ann, int Mx, int ktot, const float* cand, float* thr) {
    __shared__ float red[4];
    const int j = blockIdx.x, n = blockIdx.y;
    if (ann[((long)n * Mx + j) * 5 + 4] == -1.f) return;
    const float* c = cand + ((long)n * Mx + j) * ktot;
    float s = 0.f;
    for (int i = threadIdx.x; i < ktot; i += 256) s += c[i];
    const float mean = atss_block_sum(s, red) / (float)ktot;
    float q = 0.f;
    for (int i = threadIdx.x; i < ktot; i += 256) { const float d = c[i] - mean; q += d * d; }
    q = atss_block_sum(q, red);
    if (threadIdx.x == 0) thr[(long)n * Mx + j] = mean + (ktot > 1 ? sqrtf(q / (float)(ktot - 1)) : 0.f);
}

__global__ __launch_bounds__(256) void atss_assign_kernel(const float* anchors, const float* ann, int A, int Mx, AtssLevels L,
                                                          const unsigned long long* kth, const float* thr, short* assign) {
    const int n = blockIdx.y;
    const int a = blockIdx.x * 256 + threadIdx.x;
    if (a >= A) return;
    int l = 0;
    while (l + 1 < L.n && a >= L.off[l + 1]) ++l;
    const int idx = a - L.off[l];
    const float* anc = anchors + (long)a * 4;
    const float acy = (anc[0] + anc[2]) * 0.5f, acx = (anc[1] + anc[3]) * 0.5f;
    float best = -1.f;
    int arg = -1;
    for (int j = 0; j < Mx; ++j) {
        const float* b = ann + ((long)n * Mx + j) * 5;
        if (b[4] == -1.f) continue;
        float gcx, gcy;
        atss_box_centre(b, gcx, gcy);
        if (atss_key(atss_d2(anc, gcx, gcy), idx) > kth[((long)n * Mx + j) * L.n + l]) continue;
        const float iou = atss_iou(anc, b);
        if (!(iou >= thr[(long)n * Mx + j])) continue;
        const float side = fminf(fminf(acx - b[0], acy - b[1]), fminf(b[2] - acx, b[3] - acy));
        if (!(side > 0.01f)) continue;
        if (iou > best) { best = iou; arg = j; }                       // the lowest annotation index wins a tie
    }
    assign[(long)n * A + a] = (short)arg;
}

// host: the level table of one call; false when the sizes do not describe A anchors or a k_l does not fit the LDS lists
static bool atss_levels(const int* level_sizes, int n_levels, int A, int topk, int apl, AtssLevels& L) {
    if (!level_sizes || n_levels < 1 || n_levels > HN_ATSS_MAX_LEVELS || topk < 1 || apl < 1) return false;
    if ((long)topk * apl > HN_ATSS_MAXK) return false;
    L.n = n_levels;
    L.off[0] = 0;
    L.koff[0] = 0;
    long sum = 0;
    for (int l = 0; l < n_levels; ++l) {
        if (level_sizes[l] < 1) return false;
        sum += level_sizes[l];
        if (sum > A) return false;
        L.off[l + 1] = (int)sum;
        L.k[l] = topk * apl < level_sizes[l] ? topk * apl : level_sizes[l];
        L.koff[l + 1] = L.koff[l] + L.k[l];
    }
    return sum == A;
}

static long atss_kth_bytes(int N, int Mx, int n_levels) { return (((long)N * Mx * n_levels * 8) + 255) / 256 * 256; }

// workspace bytes of hn_det_atss_assign (level_sizes: a host array); -1 for arguments hn_det_atss_assign would reject
extern "C" long hn_det_atss_ws_bytes(int N, int A, int Mx, const int* level_sizes, int n_levels, int topk, int anchors_per_location) {
    AtssLevels L;
    if (N < 1 || A < 1 || Mx < 1 || !atss_levels(level_sizes, n_levels, A, topk, anchors_per_location, L)) return -1;
    return atss_kth_bytes(N, Mx, n_levels) + (long)N * Mx * L.koff[L.n] * 4;
}

// anchors fp32 [A][4], ann fp32 [N][Mx][5], level_sizes: HOST int [n_levels] (read during the call), ws: hn_det_atss_ws_bytes bytes;
// writes assign int16 [N][A] (>= 0 matched annotation, -1 background) and thr fp32 [N][Mx] (rows of padding annotations are not written)
extern "C" int hn_det_atss_assign(const float* anchors, const float* ann, int N, int A, int Mx, const int* level_sizes, int n_levels, int topk,
                                  int anchors_per_location, void* ws, void* assign, float* thr, hipStream_t st) {
    HN_CHECK_ARG(((uintptr_t)anchors & 15) == 0);                       // an anchor is read as one 16-byte load
    HN_CHECK_ARG(anchors && ann && ws && assign && thr && N > 0 && N <= 65535 && A > 0 && Mx > 0 && Mx <= 32767);   // int16 assign, grid z / y
    AtssLevels L;
    HN_CHECK_ARG(atss_levels(level_sizes, n_levels, A, topk, anchors_per_location, L));
    unsigned long long* kth = (unsigned long long*)ws;
    float* cand = (float*)((char*)ws + atss_kth_bytes(N, Mx, n_levels));
    hipLaunchKernelGGL(atss_select_kernel, dim3(n_levels, Mx, N), dim3(HN_ATSS_THREADS), 0, st, anchors, ann, Mx, L, kth, cand);
    hipLaunchKernelGGL(atss_thr_kernel, dim3(Mx, N), dim3(256), 0, st, ann, Mx, L.koff[L.n], (const float*)cand, thr);
    hipLaunchKernelGGL(atss_assign_kernel, dim3((A + 255) / 256, N), dim3(256), 0, st, anchors, ann, A, Mx, L, (const unsigned long long*)kth,
                       (const float*)thr, (short*)assign);
    HN_LAUNCH_CHECK();
}
