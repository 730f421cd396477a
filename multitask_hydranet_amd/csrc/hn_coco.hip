// COCO box mAP (pycocotools COCOeval(gt, dt, 'bbox') evaluate + accumulate, as head_detect/detect_eval.py calls it) on device, no host
// synchronisation.  The host (det_eval.py) packs the ground truth once per evaluator and the detections once per update; the summary of
// the 12 stats is host code over the precision / recall arrays written here.
//
// Parity rules (the numbers are compared to COCOeval's bit for bit, so every comparison below is exact):
//   * IoU is maskApi's bbIou on the xywh boxes in fp64: w = min(dx+dw, gx+gw) - max(dx, gx), h likewise (0 if either <= 0), i = w*h,
//     u = (da + ga) - i with da = dw*dh, ga = gw*gh, iou = i / u.  FMA contraction is off for the whole file (the pragma below): a fused
//     da + ga would change IoUs that are then compared to the thresholds exactly.
//   * evaluateImg per (image, category), maxDet 100: detections in stable descending score order, the first 100 kept; per area range
//     a GT is ignored when its `area` is outside [lo, hi] (inclusive bounds); for every threshold t (min(iouThr, 1 - 1e-10), from the host)
//     and every kept detection in order, the match is the unmatched GT of the best class (non-ignored before ignored, the scan's break),
//     then the highest IoU >= t, then the LATER GT on an IoU tie (the scan's `<` continue).  dtIg = the matched GT's ignore flag, or
//     (unmatched) the detection's area w*h outside the range.
//   * accumulate per (category, area, maxDets, threshold): the category's records stable-sorted by descending score, ties in (image order,
//     rank in the image); the records with rank < maxDets; tp = matched & !ignored, fp = !matched & !ignored as running counts;
//     rc = tp / npig, pr = tp / ((fp + tp) + 2^-52); precision[r] = max { pr_i : rc_i >= recThrs[r] } (= the right-to-left envelope read
//     at searchsorted_left(rc, recThrs[r]); 0 when no rc reaches it); recall = tp_total / npig; npig == 0 leaves both at -1.
//
// Kernels:
//   coco_match_kernel   one workgroup per (image, category) cell of an update; each of the T x 4 (threshold, area range) greedy passes
//                       runs on its own group of CC_SUB lanes, one detection at a time, the GT search a reduction across the group.  GTs
//                       and their matched flags are in LDS up to CC_GCAP GTs per cell, in global memory (the caller's workspace) beyond:
//                       the same code through flat pointers.  Output: one 32-byte
//                       record per kept detection {score f32, image order * 128 + rank, category, 0, per area (matched bits 0..T-1 |
//                       ignored bits 16..16+T-1)} at a position the host assigned (no atomics, no read-back).
//   coco_key_kernel     64-bit sort keys: category | descending score | image order * 128 + rank (the sequence makes the LSD sort total).
//   coco_hist / coco_scan / coco_scatter   a stable LSD radix sort of the keys, 8 bits per pass, as many passes as the key has bits.
//   coco_accum_kernel   one workgroup per (category, area, maxDets, threshold): block scans of the tp / fp counts along the sorted order,
//                       the envelope as an LDS max per recall-threshold bucket and a suffix max.
// Every sum is an integer count and every max is exact: results are bitwise reproducible.
#include "hn_common.h"

#pragma clang fp contract(off)

#define CC_THREADS 256
#define CC_MAXDET 100
#define CC_GCAP 256
#define CC_A 4
#define CC_MAXT 16
#define CC_SUB 16                     // lanes per greedy pass
#define CC_MAXR 128
#define CC_ROUNDS 8
#define CC_TILE (CC_THREADS * CC_ROUNDS)

__device__ __forceinline__ double cc_iou(const double* d, const double* g) {
    const double w = fmin(d[2] + d[0], g[2] + g[0]) - fmax(d[0], g[0]);
    if (w <= 0.0) return 0.0;
    const double h = fmin(d[3] + d[1], g[3] + g[1]) - fmax(d[1], g[1]);
    if (h <= 0.0) return 0.0;
    const double i = w * h;
    const double da = d[2] * d[3], ga = g[2] * g[3];
    const double u = (da + ga) - i;
    return i / u;
}

// candidate (class = key >> 30, iou, gt index = key & (2^30 - 1)) better than the current best?  key -1 = none.
__device__ __forceinline__ bool cc_better(int key, double iou, int bkey, double biou) {
    const int c = key >> 30, bc = bkey >> 30;
    return c > bc || (c == bc && (iou > biou || (iou == biou && key > bkey)));
}

// cells [n][4] int: {gt cell = image order * K + category, first detection, detection count, first record};
// dets [n][5] fp64: x, y, w, h, score (an fp32 value); gt [G][5] fp64: x, y, w, h, area; gt_off [cells + 1];
// prm: thresholds [T] then the area ranges [4][2].  Block = T * 4 passes x CC_SUB lanes; pass p = (threshold p / 4, area range p % 4).
__global__ __launch_bounds__(CC_MAXT * CC_A * CC_SUB) void coco_match_kernel(const int4* __restrict__ cells, const double* __restrict__ dets,
                                                                            const int* __restrict__ gt_off, const double* __restrict__ gt,
                                                                            const double* __restrict__ prm, int K, int T,
                                                                            unsigned char* gtm_ws, int* __restrict__ rec) {
    __shared__ double s_det[CC_MAXDET][6];           // x, y, w, h, score, area
    __shared__ double s_gt[CC_GCAP * 5];
    __shared__ unsigned char s_gtm[CC_MAXT * CC_A * CC_GCAP];
    __shared__ unsigned s_bits[CC_MAXDET][CC_A];
    __shared__ double s_prm[CC_MAXT + 2 * CC_A];
    const int tid = threadIdx.x, nthr = blockDim.x;
    const int p = tid / CC_SUB, sl = tid % CC_SUB, t = p / CC_A, a = p % CC_A, P = T * CC_A;
    const int4 c = cells[blockIdx.x];
    const int gc = c.x, d0 = c.y, nd = c.z, r0 = c.w;
    const int k = gc % K, img = gc / K;
    const int g0 = gt_off[gc], G = gt_off[gc + 1] - g0;
    const bool in_lds = G <= CC_GCAP;
    const double* gb = in_lds ? s_gt : gt + (long)g0 * 5;
    unsigned char* gtm = in_lds ? s_gtm : gtm_ws + (long)g0 * CC_MAXT * CC_A;     // matched flags [pass][G]
    // stable descending score rank of every detection of the cell; the first CC_MAXDET land in LDS at their rank
    for (int j = tid; j < nd; j += nthr) {
        const double* dj = dets + (long)(d0 + j) * 5;
        const double sj = dj[4];
        int r = 0;
        for (int i = 0; i < nd && r < CC_MAXDET; ++i) {
            const double si = dets[(long)(d0 + i) * 5 + 4];
            r += (si > sj) || (si == sj && i < j);
        }
        if (r < CC_MAXDET) {
#pragma unroll
            for (int q = 0; q < 5; ++q) s_det[r][q] = dj[q];
            s_det[r][5] = dj[2] * dj[3];
        }
    }
    if (in_lds)
        for (int i = tid; i < G * 5; i += nthr) s_gt[i] = gt[(long)g0 * 5 + i];
    for (int i = tid; i < G * P; i += nthr) gtm[i] = 0;
    for (int i = tid; i < CC_MAXDET * CC_A; i += nthr) (&s_bits[0][0])[i] = 0u;
    if (tid < T + 2 * CC_A) s_prm[tid] = prm[tid];
    __syncthreads();
    const int D = nd < CC_MAXDET ? nd : CC_MAXDET;
    const double thr = s_prm[t], lo = s_prm[T + 2 * a], hi = s_prm[T + 2 * a + 1];
    unsigned char* m = gtm + p * G;
    // one greedy pass per CC_SUB-lane group; every group of a wave walks the same D detections and G GTs (uniform trip counts)
    for (int d = 0; d < D; ++d) {
        const double* db = s_det[d];
        double bi = -1.0;
        int bkey = -1;
        // lane sl scans GTs sl, sl + CC_SUB, ...: it alone reads and writes their matched flags (no cross-lane memory hand-off)
        for (int g = sl; g < G; g += CC_SUB) {
            if (m[g]) continue;
            const double* gg = gb + g * 5;
            const double iou = cc_iou(db, gg);
            if (iou < thr) continue;
            const int key = ((gg[4] < lo || gg[4] > hi) ? 0 : (1 << 30)) | g;
            if (cc_better(key, iou, bkey, bi)) { bi = iou; bkey = key; }
        }
#pragma unroll
        for (int o = CC_SUB / 2; o >= 1; o >>= 1) {            // xor offsets < CC_SUB stay inside the group
            const double oi = __shfl_xor(bi, o);
            const int ok = __shfl_xor(bkey, o);
            if (cc_better(ok, oi, bkey, bi)) { bi = oi; bkey = ok; }
        }
        if (bkey >= 0) {
            const int g = bkey & ((1 << 30) - 1);
            if (sl == g % CC_SUB) m[g] = 1;
            if (sl == 0) atomicOr(&s_bits[d][a], (1u << t) | ((bkey >> 30) ? 0u : (1u << (16 + t))));
        } else if (sl == 0 && (s_det[d][5] < lo || s_det[d][5] > hi)) {
            atomicOr(&s_bits[d][a], 1u << (16 + t));
        }
    }
    __syncthreads();
    for (int d = tid; d < D; d += nthr) {
        int* o = rec + (long)(r0 + d) * 8;
        o[0] = __float_as_int((float)s_det[d][4]);
        o[1] = img * 128 + d;
        o[2] = k;
        o[3] = 0;
#pragma unroll
        for (int q = 0; q < CC_A; ++q) o[4 + q] = (int)s_bits[d][q];
    }
}

__global__ void coco_key_kernel(const int* __restrict__ rec, long N, int seq_bits, unsigned long long* __restrict__ key,
                                unsigned* __restrict__ val) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const int* r = rec + i * 8;
    unsigned u = (unsigned)r[0];
    if (__int_as_float(r[0]) == 0.0f) u = 0u;                        // -0 ties with +0, as in the host's comparison
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);                  // ascending float order
    u = ~u;                                                          // descending
    key[i] = ((unsigned long long)(unsigned)r[2] << (32 + seq_bits)) | ((unsigned long long)u << seq_bits) | (unsigned)r[1];
    val[i] = (unsigned)i;
}

__global__ __launch_bounds__(CC_THREADS) void coco_hist_kernel(const unsigned long long* __restrict__ key, long N, int shift, int ntiles,
                                                               unsigned* __restrict__ hist) {
    __shared__ unsigned h[256];
    const int tid = threadIdx.x;
    h[tid] = 0;
    __syncthreads();
    const long t0 = (long)blockIdx.x * CC_TILE;
    for (int r = 0; r < CC_ROUNDS; ++r) {
        const long i = t0 + r * CC_THREADS + tid;
        if (i < N) atomicAdd(&h[(unsigned)(key[i] >> shift) & 255u], 1u);
    }
    __syncthreads();
    hist[(long)tid * ntiles + blockIdx.x] = h[tid];
}

// exclusive scan of one value per thread over a block of NW waves; `total` = the block's sum.  sh: NW words of LDS.
template <int NW>
__device__ __forceinline__ unsigned cc_block_scan(unsigned v, unsigned* sh, unsigned& total) {
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
    for (int q = 0; q < NW; ++q) {
        const unsigned t = sh[q];
        if (q < w) pre += t;
        total += t;
    }
    __syncthreads();
    return pre + x - v;
}

// in-place exclusive scan of the digit-major histogram [256][ntiles] (one workgroup of 1024)
__global__ __launch_bounds__(1024) void coco_scan_kernel(unsigned* __restrict__ hist, long n) {
    __shared__ unsigned sh[16];
    unsigned carry = 0;
    for (long b = 0; b < n; b += 1024) {
        const long i = b + threadIdx.x;
        const unsigned v = i < n ? hist[i] : 0u;
        unsigned tot;
        const unsigned x = cc_block_scan<16>(v, sh, tot);
        if (i < n) hist[i] = carry + x;
        carry += tot;
    }
}

__global__ __launch_bounds__(CC_THREADS) void coco_scatter_kernel(const unsigned long long* __restrict__ kin, const unsigned* __restrict__ vin,
                                                                  long N, int shift, int ntiles, const unsigned* __restrict__ hist,
                                                                  unsigned long long* __restrict__ kout, unsigned* __restrict__ vout) {
    __shared__ unsigned base[256];
    __shared__ unsigned wcnt[4][256];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    base[tid] = hist[(long)tid * ntiles + blockIdx.x];
    const unsigned long long below = (1ull << lane) - 1ull;
    const long t0 = (long)blockIdx.x * CC_TILE;
    for (int r = 0; r < CC_ROUNDS; ++r) {
#pragma unroll
        for (int q = 0; q < 4; ++q) wcnt[q][tid] = 0;
        __syncthreads();
        const long i = t0 + r * CC_THREADS + tid;
        const bool act = i < N;
        const unsigned long long kv = act ? kin[i] : 0ull;
        const unsigned dig = (unsigned)(kv >> shift) & 255u;
        unsigned long long peers = __ballot(act);
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const bool bit = (dig >> b) & 1u;
            const unsigned long long m = __ballot(bit);
            peers &= bit ? m : ~m;
        }
        const unsigned lrank = (unsigned)__popcll(peers & below);
        const unsigned cnt = (unsigned)__popcll(peers);
        if (act && lrank == cnt - 1) wcnt[w][dig] = cnt;
        __syncthreads();
        if (act) {
            unsigned pos = base[dig] + lrank;
            for (int q = 0; q < w; ++q) pos += wcnt[q][dig];
            kout[pos] = kv;
            vout[pos] = vin[i];
        }
        __syncthreads();
        base[tid] += wcnt[0][tid] + wcnt[1][tid] + wcnt[2][tid] + wcnt[3][tid];
    }
}

// iprm: category starts [K + 1] in the sorted order, npig [K][4], maxDets [M].  precision [T][R][K][4][M], recall [T][K][4][M].
__global__ __launch_bounds__(CC_THREADS) void coco_accum_kernel(const int* __restrict__ rec, const unsigned* __restrict__ order, long N,
                                                                const int* __restrict__ iprm, const double* __restrict__ rthr, int K, int T,
                                                                int R, int M, double* __restrict__ precision, double* __restrict__ recall) {
    __shared__ double s_rt[CC_MAXR];
    __shared__ unsigned long long s_mx[CC_MAXR];
    __shared__ unsigned sh[4];
    const int tid = threadIdx.x;
    const int b = blockIdx.x;
    const int t = b % T, m = (b / T) % M, a = (b / (T * M)) % CC_A, k = b / (T * M * CC_A);
    const int np = iprm[K + 1 + k * CC_A + a];
    const int maxdet = iprm[K + 1 + K * CC_A + m];
    const long pidx = (((long)k * CC_A + a) * M + m);
    if (np == 0) {
        for (int r = tid; r < R; r += CC_THREADS) precision[((long)t * R + r) * K * CC_A * M + pidx] = -1.0;
        if (tid == 0) recall[(long)t * K * CC_A * M + pidx] = -1.0;
        return;
    }
    for (int r = tid; r < CC_MAXR; r += CC_THREADS) {
        s_rt[r] = r < R ? rthr[r] : 0.0;
        s_mx[r] = 0ull;                                              // bits of +0.0: the precision where no recall reaches the threshold
    }
    __syncthreads();
    const long s = iprm[k];
    long e = iprm[k + 1];
    if (e > N) e = N;
    const double npd = (double)np;
    unsigned ctp = 0, cfp = 0;
    for (long base = s; base < e; base += CC_THREADS) {
        const long i = base + tid;
        bool valid = false;
        unsigned v = 0;
        if (i < e) {
            const int* r = rec + (long)order[i] * 8;
            valid = (r[1] & 127) < maxdet;
            const unsigned bits = (unsigned)r[4 + a];
            const unsigned mt = (bits >> t) & 1u, ig = (bits >> (16 + t)) & 1u;
            if (valid && !ig) v = mt ? 1u : (1u << 16);
        }
        unsigned tot;
        const unsigned incl = cc_block_scan<4>(v, sh, tot) + v;
        if (valid) {
            const double tp = (double)(ctp + (incl & 0xffffu)), fp = (double)(cfp + (incl >> 16));
            const double rc = tp / npd;
            const double pr = tp / ((fp + tp) + 2.220446049250313e-16);
            int lo = 0, hi = R;                                      // recall thresholds <= rc: [0, lo)
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (s_rt[mid] <= rc) lo = mid + 1; else hi = mid;
            }
            if (lo > 0) atomicMax(&s_mx[lo - 1], (unsigned long long)__double_as_longlong(pr));
        }
        ctp += tot & 0xffffu;
        cfp += tot >> 16;
    }
    __syncthreads();
    for (int r = tid; r < R; r += CC_THREADS) {
        unsigned long long q = 0ull;
        for (int j = r; j < R; ++j) q = s_mx[j] > q ? s_mx[j] : q;
        precision[((long)t * R + r) * K * CC_A * M + pidx] = __longlong_as_double((long long)q);
    }
    if (tid == 0) recall[(long)t * K * CC_A * M + pidx] = (double)ctp / npd;
}

static long cc_align(long x) { return (x + 255) & ~255L; }
static long cc_tiles(long N) { return (N + CC_TILE - 1) / CC_TILE; }
static int cc_bits(long x) { int b = 0; while (x > 0) { ++b; x >>= 1; } return b; }

extern "C" long hn_coco_match_ws_bytes(long n_gt) { return n_gt > 0 ? cc_align(n_gt * CC_MAXT * CC_A) : 256; }

extern "C" int hn_coco_match(const int* cells, int n_cells, const double* dets, const int* gt_off, const double* gt, const double* prm, int K,
                             int T, void* gtm_ws, int* rec, hipStream_t stream) {
    HN_CHECK_ARG(n_cells >= 0 && K >= 1 && T >= 1 && T <= CC_MAXT);
    if (n_cells == 0) return HN_OK;
    HN_CHECK_ARG(cells && dets && gt_off && gt && prm && gtm_ws && rec);
    coco_match_kernel<<<n_cells, T * CC_A * CC_SUB, 0, stream>>>(reinterpret_cast<const int4*>(cells), dets, gt_off, gt, prm, K, T,
                                                                 static_cast<unsigned char*>(gtm_ws), rec);
    HN_LAUNCH_CHECK();
}

extern "C" long hn_coco_accumulate_ws_bytes(long N) {
    const long n = N > 0 ? N : 1;
    return 2 * cc_align(n * 8) + 2 * cc_align(n * 4) + cc_align(256 * cc_tiles(n) * 4);
}

extern "C" int hn_coco_accumulate(const int* rec, long N, int K, int seq_bits, const int* iprm, const double* rec_thrs, int T, int R, int M,
                                  void* ws, double* precision, double* recall, hipStream_t stream) {
    HN_CHECK_ARG(N >= 0 && N < (1L << 31) && K >= 1 && T >= 1 && T <= CC_MAXT && R >= 1 && R <= CC_MAXR && M >= 1);
    HN_CHECK_ARG(seq_bits >= 0 && seq_bits <= 31 && seq_bits + 32 + cc_bits(K - 1) <= 64);
    HN_CHECK_ARG(iprm && rec_thrs && ws && precision && recall && (N == 0 || rec));
    char* w = static_cast<char*>(ws);
    const long n = N > 0 ? N : 1;
    unsigned long long* ka = reinterpret_cast<unsigned long long*>(w);
    unsigned long long* kb = reinterpret_cast<unsigned long long*>(w + cc_align(n * 8));
    unsigned* va = reinterpret_cast<unsigned*>(w + 2 * cc_align(n * 8));
    unsigned* vb = reinterpret_cast<unsigned*>(w + 2 * cc_align(n * 8) + cc_align(n * 4));
    unsigned* hist = reinterpret_cast<unsigned*>(w + 2 * cc_align(n * 8) + 2 * cc_align(n * 4));
    if (N > 0) {
        const int ntiles = (int)cc_tiles(N);
        coco_key_kernel<<<(unsigned)((N + 255) / 256), 256, 0, stream>>>(rec, N, seq_bits, ka, va);
        const int passes = (seq_bits + 32 + cc_bits(K - 1) + 7) / 8;
        for (int p = 0; p < passes; ++p) {
            coco_hist_kernel<<<ntiles, CC_THREADS, 0, stream>>>(ka, N, 8 * p, ntiles, hist);
            coco_scan_kernel<<<1, 1024, 0, stream>>>(hist, 256L * ntiles);
            coco_scatter_kernel<<<ntiles, CC_THREADS, 0, stream>>>(ka, va, N, 8 * p, ntiles, hist, kb, vb);
            unsigned long long* tk = ka; ka = kb; kb = tk;
            unsigned* tv = va; va = vb; vb = tv;
        }
    }
    coco_accum_kernel<<<K * CC_A * M * T, CC_THREADS, 0, stream>>>(rec, va, N, iprm, rec_thrs, K, T, R, M, precision, recall);
    HN_LAUNCH_CHECK();
}
