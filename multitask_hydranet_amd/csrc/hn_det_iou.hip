// Detection loss with an IoU-family regression term (detection.loss_reg_type = giou | diou | ciou).  Anchor assignment and the focal
// classification loss are hn_loss.hip's (hn_det_common.h); only the regression term of the positive anchors differs: instead of smooth-L1
// on (dy, dx, dh, dw) the anchor's prediction is decoded to a box the way deploy mode decodes it (BBoxTransform,
// head_detect/detection_loss.py:19-33) and compared with its annotation.
//
//   predicted box  cy = dy ha + cya, cx = dx wa + cxa, h = exp(min(dh, C)) ha, w = exp(min(dw, C)) wa, C = log(1000/16)
//   target box     the annotation's centre, gw = max(x2 - x1, 1), gh = max(y2 - y1, 1) (the clamp of the smooth-L1 targets)
//   iou            inter / union, inter = max(0, iw) max(0, ih), union = w h + gw gh - inter + eps, eps = 1e-7
//   enclosing box  sides cw, ch
//   giou (kind 1)  1 - iou + (ac - union) / ac,        ac = cw ch + eps
//   diou (kind 2)  1 - iou + rho2 / c2,                rho2 = (cx - gcx)^2 + (cy - gcy)^2, c2 = cw^2 + ch^2 + eps
//   ciou (kind 3)  diou + alpha v,                     v = (4 / pi^2) (atan(gw / gh) - atan(w / h))^2, alpha = v / (1 - iou + v + eps),
//                                                      alpha a constant in the backward
//   per image sum_pos / npos (0 without positives), batch mean; the positives' mean iou is reduced the same way (out[2]).
//
// Same shape as the smooth-L1 kernels: one thread per (image, anchor), wave sums into per-block partial rows, a one-block finalize; no
// atomics, a fixed summation order.  The backward recomputes the box from reg / anchors / ann / assign.
#include "hn_common.h"
#include "hn_det_common.h"
#include "hn_det_iou_box.h"   // det_iou_box: shared with hn_det_quality.hip

extern "C" int hn_det_loss_blocks(int A);                             // hn_loss.hip: partial rows per image

// GIVEN: assign is an input (hn_det_loss_iou_fwd_assigned: ATSS, hn_det_atss.hip) instead of det_assign's output
template <bool GIVEN>
__global__ __launch_bounds__(256) void det_loss_iou_fwd_kernel(const float* cls, const float* reg, const float* anchors, const float* ann, int A,
                                                               int K, int Mx, int kind, short* assign, float* part /* [N][blocks][4] */,
                                                               const unsigned char* valid) {
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
        if (as != -2) s_cls = det_focal_sum(cls + ((long)n * A + a) * K, K, as >= 0 ? (int)an[as * 5 + 4] : -1);
        if (as >= 0) {
            s_pos = 1.f;
            det_iou_box<false>(reg + ((long)n * A + a) * 4, anc, an + as * 5, kind, s_reg, s_iou, nullptr);
        }
    }
    s_cls = wave_sum(s_cls); s_reg = wave_sum(s_reg); s_pos = wave_sum(s_pos); s_iou = wave_sum(s_iou);
    if ((threadIdx.x & 63) == 0) {
        red[threadIdx.x >> 6][0] = s_cls; red[threadIdx.x >> 6][1] = s_reg; red[threadIdx.x >> 6][2] = s_pos; red[threadIdx.x >> 6][3] = s_iou;
    }
    __syncthreads();
    if (threadIdx.x < 4) part[((long)n * gridDim.x + blockIdx.x) * 4 + threadIdx.x] =
        red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
}

__global__ __launch_bounds__(256) void det_loss_iou_bwd_kernel(const float* cls, const float* reg, const float* anchors, const float* ann, int N,
                                                               int A, int K, int Mx, int kind, const short* assign, const float* npos,
                                                               const float* gout /* [2] */, float* dcls, float* dreg,
                                                               const unsigned char* valid) {
    // the classification tile moves through LDS as in det_loss_bwd_kernel (hn_loss.hip)
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
    // (a given assignment keeps its values for an unlabelled image; a stray value counts as ignored here as in the forward, so it never
    // indexes the annotations)
    const int as = a < A && lab ? det_given_assign(assign[(long)n * A + a], Mx) : -2;
    const float* an = ann + (long)n * Mx * 5;
    if (a < A)
        det_focal_grad_row(tile + threadIdx.x * K, K, as, as >= 0 ? (int)an[as * 5 + 4] : -1, fc);
    __syncthreads();
    float* dblk = dcls + ((long)n * A + a0) * K;
    for (int i = threadIdx.x; i < nv * K; i += 256) dblk[i] = tile[i];
    if (a >= A) return;
    float g[4] = {0.f, 0.f, 0.f, 0.f};
    if (as >= 0) {
        float loss, iou;
        det_iou_box<true>(reg + ((long)n * A + a) * 4, anchors + (long)a * 4, an + as * 5, kind, loss, iou, g);
    }
    *reinterpret_cast<f32x4*>(dreg + ((long)n * A + a) * 4) = f32x4{fr * g[0], fr * g[1], fr * g[2], fr * g[3]};
}

// fwd: out[0] = classification loss, out[1] = regression loss, out[2] = mean IoU of the positives (batch means of per-image means);
// assign int16 [N][A], part fp32 [N][blocks][4], npos fp32 [N]  (valid: the det row of the task masks; nullptr = every image labelled)
static int det_loss_iou_fwd(const float* cls, const float* reg, const float* anchors, const float* ann, int N, int A, int K, int Mx,
                            int kind, void* assign, float* part, float* npos, float* out, const unsigned char* valid, hipStream_t st) {
    HN_CHECK_ARG(cls && reg && anchors && ann && assign && part && npos && out && N > 0 && A > 0 && K > 0 && K <= HN_DET_MAXK && Mx > 0);
    HN_CHECK_ARG(kind >= 1 && kind <= 3);
    const int blocks = hn_det_loss_blocks(A);
    hipLaunchKernelGGL(det_loss_iou_fwd_kernel<false>, dim3(blocks, N), dim3(256), 0, st, cls, reg, anchors, ann, A, K, Mx, kind, (short*)assign, part, valid);
    hipLaunchKernelGGL((det_loss_finalize_kernel<4, 1>), dim3(1), dim3(1024), 0, st, part, blocks, N, npos, out, valid);
    HN_LAUNCH_CHECK();
}

extern "C" int hn_det_loss_iou_fwd(const float* cls, const float* reg, const float* anchors, const float* ann, int N, int A, int K, int Mx,
                                   int kind, void* assign, float* part, float* npos, float* out, hipStream_t st) {
    return det_loss_iou_fwd(cls, reg, anchors, ann, N, A, K, Mx, kind, assign, part, npos, out, nullptr, st);
}
extern "C" int hn_det_loss_iou_fwd_masked(const float* cls, const float* reg, const float* anchors, const float* ann, int N, int A, int K,
                                          int Mx, int kind, const unsigned char* valid, void* assign, float* part, float* npos, float* out,
                                          hipStream_t st) {
    HN_CHECK_ARG(valid);
    return det_loss_iou_fwd(cls, reg, anchors, ann, N, A, K, Mx, kind, assign, part, npos, out, valid, st);
}

// hn_det_loss_iou_fwd with assign [N][A] as an INPUT (values outside -2 .. Mx - 1 count as ignored); everything else as above
static int det_loss_iou_fwd_assigned(const float* cls, const float* reg, const float* anchors, const float* ann, int N, int A, int K,
                                     int Mx, int kind, const void* assign, float* part, float* npos, float* out, const unsigned char* valid,
                                     hipStream_t st) {
    HN_CHECK_ARG(cls && reg && anchors && ann && assign && part && npos && out && N > 0 && A > 0 && K > 0 && K <= HN_DET_MAXK && Mx > 0);
    HN_CHECK_ARG(kind >= 1 && kind <= 3);
    const int blocks = hn_det_loss_blocks(A);
    hipLaunchKernelGGL(det_loss_iou_fwd_kernel<true>, dim3(blocks, N), dim3(256), 0, st, cls, reg, anchors, ann, A, K, Mx, kind, (short*)assign, part, valid);
    hipLaunchKernelGGL((det_loss_finalize_kernel<4, 1>), dim3(1), dim3(1024), 0, st, part, blocks, N, npos, out, valid);
    HN_LAUNCH_CHECK();
}

extern "C" int hn_det_loss_iou_fwd_assigned(const float* cls, const float* reg, const float* anchors, const float* ann, int N, int A, int K,
                                            int Mx, int kind, const void* assign, float* part, float* npos, float* out, hipStream_t st) {
    return det_loss_iou_fwd_assigned(cls, reg, anchors, ann, N, A, K, Mx, kind, assign, part, npos, out, nullptr, st);
}
extern "C" int hn_det_loss_iou_fwd_assigned_masked(const float* cls, const float* reg, const float* anchors, const float* ann, int N, int A,
                                                   int K, int Mx, int kind, const unsigned char* valid, const void* assign, float* part,
                                                   float* npos, float* out, hipStream_t st) {
    HN_CHECK_ARG(valid);
    return det_loss_iou_fwd_assigned(cls, reg, anchors, ann, N, A, K, Mx, kind, assign, part, npos, out, valid, st);
}

static int det_loss_iou_bwd(const float* cls, const float* reg, const float* anchors, const float* ann, int N, int A, int K, int Mx,
                            int kind, const void* assign, const float* npos, const float* gout, float* dcls, float* dreg,
                            const unsigned char* valid, hipStream_t st) {
    HN_CHECK_ARG(cls && reg && anchors && ann && assign && npos && gout && dcls && dreg && N > 0 && A > 0 && K > 0 && Mx > 0);
    HN_CHECK_ARG(K <= HN_DET_MAXK);                                     // 256 x K floats of LDS
    HN_CHECK_ARG(kind >= 1 && kind <= 3);
    hipLaunchKernelGGL(det_loss_iou_bwd_kernel, dim3(hn_det_loss_blocks(A), N), dim3(256), 256 * (size_t)K * sizeof(float), st, cls, reg, anchors,
                       ann, N, A, K, Mx, kind, (const short*)assign, npos, gout, dcls, dreg, valid);
    HN_LAUNCH_CHECK();
}
extern "C" int hn_det_loss_iou_bwd(const float* cls, const float* reg, const float* anchors, const float* ann, int N, int A, int K, int Mx,
                                   int kind, const void* assign, const float* npos, const float* gout, float* dcls, float* dreg,
                                   hipStream_t st) {
    return det_loss_iou_bwd(cls, reg, anchors, ann, N, A, K, Mx, kind, assign, npos, gout, dcls, dreg, nullptr, st);
}
extern "C" int hn_det_loss_iou_bwd_masked(const float* cls, const float* reg, const float* anchors, const float* ann, int N, int A, int K,
                                          int Mx, int kind, const unsigned char* valid, const void* assign, const float* npos,
                                          const float* gout, float* dcls, float* dreg, hipStream_t st) {
    HN_CHECK_ARG(valid);
    return det_loss_iou_bwd(cls, reg, anchors, ann, N, A, K, Mx, kind, assign, npos, gout, dcls, dreg, valid, st);
}
