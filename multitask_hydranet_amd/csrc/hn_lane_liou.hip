// Lane line-IoU regression loss (Zheng et al., CLRNet, CVPR 2022, section 3.4) on this head's encoding: the lane counterpart of the IoU
// box losses of hn_det_loss.hip.  The loss of lane.loss_loc_type: liou; hn_loss.hip's lane_loc kernels stay the smooth-L1 path.
//
// pred / target fp32 [M][L], L = 2 P + 2: columns [0, P) the x-offsets of the down part, P and P + 1 the two lengths, [P + 2, 2 P + 2) the
// x-offsets of the up part; a column is valid iff target != 0 (the reference's rule).  With the half width e > 0 in target units, for a
// positive row r (pmask[r] != 0), X_r its valid x-columns, n_r = |X_r|, d_c = |p_c - t_c|:
//   I_r = sum_X (2e - d_c)   (signed: disjoint segments count negative, as in the paper)      U_r = sum_X (2e + d_c)
//   liou_r = I_r / U_r in (-1, 1];   row_r = 1 - liou_r = 2 sum_X d_c / U_r  (the form computed: no cancellation near liou = 1), 0 if n_r = 0
//   len_r  = sum_{c in {P, P+1}, t_c != 0} alpha huber(p_c - t_c) / nrm_r,  nrm_r = max(#{c : t_c != 0 over all L columns}, 1)
//   out[0] = sum_{r positive} (row_r + len_r) / aux[1]          out[1] = mean of liou_r over the positive rows with n_r > 0 (0 without one)
// aux[1] = max(#pos, 1) of the lane classification loss; pmask / aux of hn_lane_cls_loss_fwd_masked already carry a task mask.
// Gradient: x-columns sign(p - t) 4 e n_r / U_r^2 / aux[1] gout, length columns the smooth-L1 gradient, every other element exactly 0.
//
// Launches: a row kernel (8 rows x 32 lanes per 256-thread block, a shuffle tree per row) + a one-block finalize forward, one row kernel
// backward -- the launch count of the smooth-L1 path.  No atomics, fixed summation order, nothing allocates or synchronises.
#include "hn_common.h"

// One row per group of 32 lanes.  The xor tree from offset 16 down never crosses a multiple of 32, so the two rows that share a 64-lane
// wave reduce side by side; no lane leaves before the shuffles.
__global__ __launch_bounds__(256) void lane_liou_fwd_kernel(const float* pred, const float* tgt, const unsigned char* pmask, long M, int L, int P,
                                                            float e, float alpha, float* rowI, float* rowU, float* rownorm, float* rowloss) {
    const int lane = threadIdx.x & 31, rr = threadIdx.x >> 5;
    const long r = (long)blockIdx.x * 8 + rr;
    float sd = 0.f, n = 0.f, cnt = 0.f, sl = 0.f;
    if (r < M) {
        const bool pos = pmask[r] != 0;
        const float* pr = pred + r * L;
        const float* tr = tgt + r * L;
        for (int c = lane; c < L; c += 32) {
            const float t = tr[c];
            if (t != 0.f) {
                cnt += 1.f;
                if (pos) {
                    const float d = pr[c] - t, ad = fabsf(d);
                    if (c == P || c == P + 1) {
                        sl += (ad < 1.f ? 0.5f * d * d : ad - 0.5f) * alpha;
                    } else {
                        sd += ad;
                        n += 1.f;
                    }
                }
            }
        }
    }
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) {
        sd += __shfl_xor(sd, o); n += __shfl_xor(n, o); cnt += __shfl_xor(cnt, o); sl += __shfl_xor(sl, o);
    }
    if (lane == 0 && r < M) {
        const float nrm = fmaxf(cnt, 1.f), w = 2.f * e * n, U = w + sd;
        rownorm[r] = nrm;
        rowI[r] = w - sd;
        rowU[r] = U;                                             // > 0 iff the row is positive and has a valid x-column
        rowloss[r] = (n > 0.f ? 2.f * sd / U : 0.f) + sl / nrm;
    }
}
__global__ __launch_bounds__(1024) void lane_liou_finalize_kernel(const float* rowloss, const float* rowI, const float* rowU, long M,
                                                                  const float* aux, float* out) {
    __shared__ float red[16];
    float s = 0.f, q = 0.f, k = 0.f;
    for (long i = threadIdx.x; i < M; i += 1024) {
        s += rowloss[i];
        const float u = rowU[i];
        if (u > 0.f) { q += rowI[i] / u; k += 1.f; }
    }
    s = block_sum_1024(s, red);
    q = block_sum_1024(q, red);
    k = block_sum_1024(k, red);
    if (threadIdx.x == 0) {
        out[0] = s / aux[1];
        out[1] = q / fmaxf(k, 1.f);
    }
}
// One row per group of 32 lanes again: a row that is not positive (most rows) is zero-filled without a read of pred or target.  n_r is
// the row's normaliser less its valid length columns (at a valid x-column the normaliser is the count itself, not the clamp).
__global__ __launch_bounds__(256) void lane_liou_bwd_kernel(const float* pred, const float* tgt, const unsigned char* pmask, const float* rowU,
                                                            const float* rownorm, const float* aux, const float* gout, long M, int L, int P,
                                                            float e, float alpha, float* dpred) {
    const int lane = threadIdx.x & 31, rr = threadIdx.x >> 5;
    const long r = (long)blockIdx.x * 8 + rr;
    if (r >= M) return;
    float* dr = dpred + r * L;
    if (!pmask[r]) {
        for (int c = lane; c < L; c += 32) dr[c] = 0.f;
        return;
    }
    const float* pr = pred + r * L;
    const float* tr = tgt + r * L;
    const float nrm = rownorm[r], U = rowU[r], posn = aux[1], g = gout[0];
    const float n = nrm - (tr[P] != 0.f ? 1.f : 0.f) - (tr[P + 1] != 0.f ? 1.f : 0.f);
    const float gx = U > 0.f ? 4.f * e * n / (U * U) / posn * g : 0.f;
    for (int c = lane; c < L; c += 32) {
        const float t = tr[c];
        float v = 0.f;
        if (t != 0.f) {
            const float d = pr[c] - t;
            if (c == P || c == P + 1) {
                const float dh = fabsf(d) < 1.f ? d : (d > 0.f ? 1.f : -1.f);
                v = dh * alpha / nrm / posn * g;
            } else {
                v = d > 0.f ? gx : (d < 0.f ? -gx : 0.f);
            }
        }
        dr[c] = v;
    }
}

static inline bool liou_shape_ok(long M, int L, int P, float e) {
    return M > 0 && P >= 1 && L == 2 * P + 2 && e > 0.f && e <= 3.0e38f;      // (a NaN e fails e > 0)
}
extern "C" int hn_lane_liou_loss_fwd(const float* pred, const float* target, const void* pmask, const float* aux, long M, int L, int P, float e,
                                     float alpha, float* rowI, float* rowU, float* rownorm, float* rowloss, float* out, hipStream_t st) {
    HN_CHECK_ARG(pred && target && pmask && aux && rowI && rowU && rownorm && rowloss && out && liou_shape_ok(M, L, P, e));
    hipLaunchKernelGGL(lane_liou_fwd_kernel, dim3((unsigned)((M + 7) / 8)), dim3(256), 0, st, pred, target, (const unsigned char*)pmask, M, L, P,
                       e, alpha, rowI, rowU, rownorm, rowloss);
    hipLaunchKernelGGL(lane_liou_finalize_kernel, dim3(1), dim3(1024), 0, st, rowloss, rowI, rowU, M, aux, out);
    HN_LAUNCH_CHECK();
}
extern "C" int hn_lane_liou_loss_bwd(const float* pred, const float* target, const void* pmask, const float* rowU, const float* rownorm,
                                     const float* aux, const float* gout, long M, int L, int P, float e, float alpha, float* dpred,
                                     hipStream_t st) {
    HN_CHECK_ARG(pred && target && pmask && rowU && rownorm && aux && gout && dpred && liou_shape_ok(M, L, P, e));
    hipLaunchKernelGGL(lane_liou_bwd_kernel, dim3((unsigned)((M + 7) / 8)), dim3(256), 0, st, pred, target, (const unsigned char*)pmask, rowU,
                       rownorm, aux, gout, M, L, P, e, alpha, dpred);
    HN_LAUNCH_CHECK();
}
