// Detection loss with a quality classification term (detection.loss_cls_type = qfl | vfl) next to an IoU-family regression term
// (detection.loss_reg_type = giou | diou | ciou).  Anchor assignment is hn_det_common.h's, the box function and the whole regression half
// are hn_det_iou.hip's (hn_det_iou_box.h); only the classification half differs: the target of a positive anchor's class is not 1 but the
// IoU q between the anchor's decoded prediction and its annotation -- the `iou` of det_iou_box, which the regression term computes anyway.
//
//   counted anchor (assignment != -2), class k:  y = q if the anchor is positive and k is its annotation's class, else 0
//   p^ = clamp(p, 1e-4, 1 - 1e-4) (the focal loss's clamp; zero slope outside the open range),  BCE = -(y ln p^ + (1 - y) ln(1 - p^))
//   qfl (cls_kind 1, beta 2)               l = (y - p^)^2 BCE           dl/dp = 2 (p - y) BCE + (p - y)^2 ((1 - y) / (1 - p) - y / p)
//   vfl (cls_kind 2, alpha 0.75, gamma 2)  l = y BCE            (y > 0) dl/dp = y ((1 - y) / (1 - p) - y / p)
//                                          l = 0.75 p^2 (-ln(1 - p^))   dl/dp = 0.75 (-2 p ln(1 - p) + p^2 / (1 - p))       (y = 0)
//   q is a constant in the backward: the classification term sends no gradient to the regression.
//   per image sum / max(npos, 1), mean over the (labelled) images: the focal term's reduction.
//
// At y = 0 qfl is p^2 (-ln(1 - p^)), so both kinds share one background branch up to vfl's 0.75, and that branch is the focal loss's
// background term with the fast log the focal loss uses.  The one entry per positive anchor with y > 0 uses the precise log: on a batch
// whose background is quiet those few entries ARE the loss.
//
// Same shape as hn_det_iou.hip: one thread per (image, anchor), wave sums into per-block partial rows {cls, reg, #pos, iou}, the shared
// one-block finalize; the backward stages the block's 256 x K probabilities through LDS and recomputes the box -- and with it q, from the
// same device function on the same inputs as the forward -- from reg / anchors / ann / assign.  No atomics, a fixed summation order.
#include "hn_common.h"
#include "hn_det_common.h"
#include "hn_det_iou_box.h"

extern "C" int hn_det_loss_blocks(int A);                             // hn_loss.hip: partial rows per image

// sum over the K classes of one counted anchor; cid = its class (-1 for background), q = its quality (0 for background).  The loop over
// the classes is the background branch alone and free of control flow, so its loads run ahead as in det_focal_sum; the one entry with
// y > 0 is added after it.
__device__ __forceinline__ float det_quality_sum(const float* c, int K, int cid, float q, int cls_kind) {
    const float w0 = cls_kind == 2 ? 0.75f : 1.f;
    const bool hit = q > 0.f && cid >= 0 && cid < K;                   // (a class id outside 0 .. K - 1 matches no k)
    float s = 0.f;
    for (int k = 0; k < K; ++k) {
        const float p = fminf(fmaxf(c[k], 1e-4f), 1.f - 1e-4f);
        const float bg = w0 * p * p * -__logf(1.f - p);
        s += hit && k == cid ? 0.f : bg;
    }
    if (hit) {
        const float p = fminf(fmaxf(c[cid], 1e-4f), 1.f - 1e-4f);
        const float bce = -(q * logf(p) + (1.f - q) * logf(1.f - p));
        s += cls_kind == 2 ? q * bce : (q - p) * (q - p) * bce;
    }
    return s;
}

// The classification half of the backward for one anchor, as det_focal_grad_row: c[] <- fc * d(quality sum)/dp
__device__ __forceinline__ void det_quality_grad_row(float* c, int K, int as, int cid, float q, int cls_kind, float fc) {
    const float w0 = cls_kind == 2 ? 0.75f : 1.f;
    const bool hit = as >= 0 && q > 0.f && cid >= 0 && cid < K;
    const float pq = hit ? c[cid] : 0.5f;                              // the entry with y > 0, read before the loop overwrites it
    for (int k = 0; k < K; ++k) {
        float g = 0.f;
        const float p = c[k];
        if (as != -2 && p > 1e-4f && p < 1.f - 1e-4f)                  // the clamp has zero slope outside its range
            g = w0 * (-2.f * p * __logf(1.f - p) + p * p / (1.f - p));
        c[k] = fc * g;
    }
    if (hit) {
        float g = 0.f;
        if (pq > 1e-4f && pq < 1.f - 1e-4f) {
            const float t = (1.f - q) / (1.f - pq) - q / pq;           // d BCE / dp
            if (cls_kind == 2) {
                g = q * t;
            } else {
                const float bce = -(q * logf(pq) + (1.f - q) * logf(1.f - pq));
                g = 2.f * (pq - q) * bce + (pq - q) * (pq - q) * t;
            }
        }
        c[cid] = fc * g;
    }
}

// GIVEN: assign is an input (ATSS, hn_det_atss.hip) instead of det_assign's output
template <bool GIVEN>
__global__ __launch_bounds__(256) void det_loss_quality_fwd_kernel(const float* cls, const float* reg, const float* anchors, const float* ann,
                                                                   int A, int K, int Mx, int kind, int cls_kind, short* assign,
                                                                   float* part /* [N][blocks][4] */, const unsigned char* valid) {
    __shared__ float red[4][4];
    const int n = blockIdx.y;
    const int a = blockIdx.x * 256 + threadIdx.x;
    float s_cls = 0.f, s_reg = 0.f, s_pos = 0.f, s_iou = 0.f;
    if (a < A) {
        const float* anc = anchors + (long)a * 4;
        const float* an = ann + (long)n * Mx * 5;
        int as = -2;                                                   // an unlabelled image: every anchor ignored
        if (GIVEN) {
            if (hn_image_valid(valid, n)) as = det_given_assign(assign[(long)n * A + a], Mx);
        } else {
            float biou;
            if (hn_image_valid(valid, n)) as = det_assign(anc, an, Mx, biou);
            assign[(long)n * A + a] = (short)as;
        }
        if (as >= 0) {
            s_pos = 1.f;
            det_iou_box<false>(reg + ((long)n * A + a) * 4, anc, an + as * 5, kind, s_reg, s_iou, nullptr);
        }
        if (as != -2) s_cls = det_quality_sum(cls + ((long)n * A + a) * K, K, as >= 0 ? (int)an[as * 5 + 4] : -1, s_iou, cls_kind);
    }
    s_cls = wave_sum(s_cls); s_reg = wave_sum(s_reg); s_pos = wave_sum(s_pos); s_iou = wave_sum(s_iou);
    if ((threadIdx.x & 63) == 0) {
        red[threadIdx.x >> 6][0] = s_cls; red[threadIdx.x >> 6][1] = s_reg; red[threadIdx.x >> 6][2] = s_pos; red[threadIdx.x >> 6][3] = s_iou;
    }
    __syncthreads();
    if (threadIdx.x < 4) part[((long)n * gridDim.x + blockIdx.x) * 4 + threadIdx.x] =
        red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
}

__global__ __launch_bounds__(256) void det_loss_quality_bwd_kernel(const float* cls, const float* reg, const float* anchors, const float* ann,
                                                                   int N, int A, int K, int Mx, int kind, int cls_kind, const short* assign,
                                                                   const float* npos, const float* gout /* [2] */, float* dcls, float* dreg,
                                                                   const unsigned char* valid) {
    // the classification tile moves through LDS as in det_loss_iou_bwd_kernel; every thread of the block reaches both barriers
    extern __shared__ float tile[];                                    // [256][K]
    const int n = blockIdx.y;
    const int a0 = blockIdx.x * 256;
    const int a = a0 + threadIdx.x;
    const int nv = A - a0 < 256 ? A - a0 : 256;
    const float* cblk = cls + ((long)n * A + a0) * K;
    for (int i = threadIdx.x; i < nv * K; i += 256) tile[i] = cblk[i];
    __syncthreads();
    const float p_n = npos[n];
    const bool lab = hn_image_valid(valid, n);
    const int nlab = hn_count_valid(valid, N);                         // (lab implies nlab >= 1)
    const float fc = lab ? gout[0] / (nlab * fmaxf(p_n, 1.f)) : 0.f;
    const float fr = lab && p_n > 0.f ? gout[1] / (nlab * p_n) : 0.f;
    // (a given assignment keeps its values for an unlabelled image; a stray value counts as ignored, as in the forward)
    const int as = a < A && lab ? det_given_assign(assign[(long)n * A + a], Mx) : -2;
    const float* an = ann + (long)n * Mx * 5;
    float g[4] = {0.f, 0.f, 0.f, 0.f};
    float q = 0.f;
    if (as >= 0) {                                                     // the box first: its iou is the classification target
        float loss;
        det_iou_box<true>(reg + ((long)n * A + a) * 4, anchors + (long)a * 4, an + as * 5, kind, loss, q, g);
    }
    if (a < A)
        det_quality_grad_row(tile + threadIdx.x * K, K, as, as >= 0 ? (int)an[as * 5 + 4] : -1, q, cls_kind, fc);
    __syncthreads();
    float* dblk = dcls + ((long)n * A + a0) * K;
    for (int i = threadIdx.x; i < nv * K; i += 256) dblk[i] = tile[i];
    if (a >= A) return;
    *reinterpret_cast<f32x4*>(dreg + ((long)n * A + a) * 4) = f32x4{fr * g[0], fr * g[1], fr * g[2], fr * g[3]};
}

// out[0] = classification loss (qfl / vfl), out[1] = regression loss, out[2] = mean IoU of the positives; assign int16 [N][A] (written
// unless assign_given), part fp32 [N][blocks][4], npos fp32 [N]; valid: the det row of the task masks or nullptr
extern "C" int hn_det_loss_quality_fwd(const float* cls, const float* reg, const float* anchors, const float* ann, int N, int A, int K, int Mx,
                                       int kind, int cls_kind, const unsigned char* valid, int assign_given, void* assign, float* part,
                                       float* npos, float* out, hipStream_t st) {
    HN_CHECK_ARG(cls && reg && anchors && ann && assign && part && npos && out && N > 0 && A > 0 && K > 0 && K <= HN_DET_MAXK && Mx > 0);
    HN_CHECK_ARG(kind >= 1 && kind <= 3 && cls_kind >= 1 && cls_kind <= 2 && (assign_given == 0 || assign_given == 1));
    const int blocks = hn_det_loss_blocks(A);
    if (assign_given)
        hipLaunchKernelGGL(det_loss_quality_fwd_kernel<true>, dim3(blocks, N), dim3(256), 0, st, cls, reg, anchors, ann, A, K, Mx, kind, cls_kind,
                           (short*)assign, part, valid);
    else
        hipLaunchKernelGGL(det_loss_quality_fwd_kernel<false>, dim3(blocks, N), dim3(256), 0, st, cls, reg, anchors, ann, A, K, Mx, kind, cls_kind,
                           (short*)assign, part, valid);
    hipLaunchKernelGGL((det_loss_finalize_kernel<4, 1>), dim3(1), dim3(1024), 0, st, part, blocks, N, npos, out, valid);
    HN_LAUNCH_CHECK();
}

extern "C" int hn_det_loss_quality_bwd(const float* cls, const float* reg, const float* anchors, const float* ann, int N, int A, int K, int Mx,
                                       int kind, int cls_kind, const unsigned char* valid, const void* assign, const float* npos,
                                       const float* gout, float* dcls, float* dreg, hipStream_t st) {
    HN_CHECK_ARG(cls && reg && anchors && ann && assign && npos && gout && dcls && dreg && N > 0 && A > 0 && K > 0 && Mx > 0);
    HN_CHECK_ARG(K <= HN_DET_MAXK);                                     // 256 x K floats of LDS
    HN_CHECK_ARG(kind >= 1 && kind <= 3 && cls_kind >= 1 && cls_kind <= 2);
    hipLaunchKernelGGL(det_loss_quality_bwd_kernel, dim3(hn_det_loss_blocks(A), N), dim3(256), 256 * (size_t)K * sizeof(float), st, cls, reg,
                       anchors, ann, N, A, K, Mx, kind, cls_kind, (const short*)assign, npos, gout, dcls, dreg, valid);
    HN_LAUNCH_CHECK();
}
