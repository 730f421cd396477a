// The detection loss: one forward and one backward kernel for every combination of its regression term (detection.loss_reg_type =
// smooth_l1 | giou | diou | ciou) and its classification term (detection.loss_cls_type = focal | qfl | vfl), with the assignment computed
// in the launch or handed in, with or without a task mask.  The kernels are templates over <IOU, QUALITY[, GIVEN]>; the two terms are
// the four device functions below and the only places where the instantiations differ.  Assignment, the mask helpers and the finalize
// kernel are hn_det_common.h's.
//
// ---------------------------------------------------------------------------------------------------------
// Detection loss (FocalLoss.forward, head_detect/detection_loss.py:132-267): IoU assignment (neg < 0.4, pos >= 0.5, else ignored),
// focal BCE (alpha 0.25, gamma 2) on probabilities clamped to [1e-4, 1-1e-4] divided by max(#pos, 1), smooth-L1 (beta 1/9) on
// (dy, dx, dh, dw) averaged over positives x 4; batch mean.  One thread per (image, anchor); the per-image Python loop and the
// A x M IoU matrix of the reference never exist.  assign[n][a]: >= 0 matched annotation, -1 background, -2 ignored.
// ---------------------------------------------------------------------------------------------------------
//
// Detection loss with an IoU-family regression term (detection.loss_reg_type = giou | diou | ciou).  Anchor assignment and the focal
// classification loss are the smooth-L1 loss's; only the regression term of the positive anchors differs: instead of smooth-L1
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
// Detection loss with a quality classification term (detection.loss_cls_type = qfl | vfl) next to an IoU-family regression term
// (detection.loss_reg_type = giou | diou | ciou).  Anchor assignment, the box function and the whole regression half are the ones
// above; only the classification half differs: the target of a positive anchor's class is not 1 but the
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
// One shape for all of them: one thread per (image, anchor), wave sums into per-block partial rows {cls, reg, #pos[, iou]}, the shared
// one-block finalize; the backward stages the block's 256 x K probabilities through LDS and recomputes the regression term -- and with
// the box its q, from the same device function on the same inputs as the forward -- from reg / anchors / ann / assign.  No atomics, a
// fixed summation order.
#include "hn_common.h"
#include "hn_det_common.h"

// ---- regression terms of one positive anchor: r = its (dy, dx, dh, dw), anc = its anchor, b = its annotation ----

// smooth-L1 against the encoded target: without GRAD loss = the sum over the four coordinates, with GRAD g[4] = d loss / d r (loss is
// left alone)
template <bool GRAD>
__device__ __forceinline__ void det_smooth_l1(const float* r, const float* anc, const float* b, float& loss, float* g) {
    const float aw = anc[3] - anc[1], ah = anc[2] - anc[0];
    const float acx = anc[1] + 0.5f * aw, acy = anc[0] + 0.5f * ah;
    float gw = b[2] - b[0], gh = b[3] - b[1];
    const float gcx = b[0] + 0.5f * gw, gcy = b[1] + 0.5f * gh;
    gw = fmaxf(gw, 1.f);
    gh = fmaxf(gh, 1.f);
    const float t[4] = {(gcy - acy) / ah, (gcx - acx) / aw, __logf(gh / ah), __logf(gw / aw)};
    if (!GRAD) loss = 0.f;
    for (int q = 0; q < 4; ++q) {
        if (GRAD) {
            const float d = t[q] - r[q];
            const float ad = fabsf(d);
            g[q] = ad <= 1.f / 9.f ? -9.f * d : (d > 0.f ? -1.f : 1.f);
        } else {
            const float d = fabsf(t[q] - r[q]);
            loss += d <= 1.f / 9.f ? 0.5f * 9.f * d * d : d - 0.5f / 9.f;
        }
    }
}

// (the box function of the IoU-family terms, det_iou_box, is hn_det_common.h's: the task-aligned assigner measures with it too)

// ---- classification terms of one counted anchor: c = its K probabilities, cid = its class (-1 for background) ----

// focal BCE (alpha 0.25, gamma 2) of the K probabilities, clamped to [1e-4, 1-1e-4]
__device__ __forceinline__ float det_focal_sum(const float* c, int K, int cid) {
    float s = 0.f;
    for (int k = 0; k < K; ++k) {
        const float p = fminf(fmaxf(c[k], 1e-4f), 1.f - 1e-4f);
        if (k == cid) s += 0.25f * (1.f - p) * (1.f - p) * -__logf(p);
        else s += 0.75f * p * p * -__logf(1.f - p);
    }
    return s;
}

// The classification half of the backward for one anchor: its K probabilities in c[] are replaced by fc * d(focal sum)/dp.  as = the
// anchor's assignment.  The backward kernel stages the block's 256 x K run through LDS and hands each thread its own row.
__device__ __forceinline__ void det_focal_grad_row(float* c, int K, int as, int cid, float fc) {
    for (int k = 0; k < K; ++k) {
        float g = 0.f;
        const float p = c[k];
        if (as != -2 && p > 1e-4f && p < 1.f - 1e-4f) {                // the clamp has zero slope outside its range
            if (k == cid) g = 0.25f * (2.f * (1.f - p) * __logf(p) - (1.f - p) * (1.f - p) / p);
            else g = 0.75f * (-2.f * p * __logf(1.f - p) + p * p / (1.f - p));
        }
        c[k] = fc * g;
    }
}

// the quality sum (qfl / vfl) over the K classes; q = the anchor's quality (0 for background).  The loop over
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

// ---- the kernel pair ----
// IOU: the regression term is det_iou_box (kind 1..3) and the partial rows carry the positives' iou as a fourth column, else
// det_smooth_l1 and three columns (kind unused).  QUALITY (only with IOU): the classification term is det_quality_sum (cls_kind 1..2)
// with the box's iou as its target, else det_focal_sum (cls_kind unused).  GIVEN: assign is an input (ATSS, hn_det_atss.hip) instead of
// det_assign's output.
template <bool IOU, bool QUALITY, bool GIVEN>
__global__ __launch_bounds__(256) void det_loss_fwd_kernel(const float* cls, const float* reg, const float* anchors, const float* ann, int A,
                                                           int K, int Mx, int kind, int cls_kind, short* assign,
                                                           float* part /* [N][blocks][COLS] */, const unsigned char* valid,
                                                           const float* target /* [N][A] or nullptr (QUALITY only) */) {
    static_assert(IOU || !QUALITY, "the quality terms' target is the box's iou");
    constexpr int COLS = IOU ? 4 : 3;
    __shared__ float red[4][COLS];
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
        if (as >= 0) {                                                 // the box first: its iou is the quality terms' target
            s_pos = 1.f;
            const float* r = reg + ((long)n * A + a) * 4;
            if (IOU) det_iou_box<false>(r, anc, an + as * 5, kind, s_reg, s_iou, nullptr);
            else det_smooth_l1<false>(r, anc, an + as * 5, s_reg, nullptr);
        }
        if (as != -2) {
            const float* c = cls + ((long)n * A + a) * K;
            const int cid = as >= 0 ? (int)an[as * 5 + 4] : -1;
            if (QUALITY) {                                             // a given target (hn_det_tal.hip's) replaces the positives' iou as y
                const float y = target && as >= 0 ? target[(long)n * A + a] : s_iou;
                s_cls = det_quality_sum(c, K, cid, y, cls_kind);
            } else {
                s_cls = det_focal_sum(c, K, cid);
            }
        }
    }
    s_cls = wave_sum(s_cls); s_reg = wave_sum(s_reg); s_pos = wave_sum(s_pos);
    if (IOU) s_iou = wave_sum(s_iou);
    if ((threadIdx.x & 63) == 0) {
        red[threadIdx.x >> 6][0] = s_cls; red[threadIdx.x >> 6][1] = s_reg; red[threadIdx.x >> 6][2] = s_pos;
        if (IOU) red[threadIdx.x >> 6][COLS - 1] = s_iou;
    }
    __syncthreads();
    if (threadIdx.x < COLS) part[((long)n * gridDim.x + blockIdx.x) * COLS + threadIdx.x] =
        red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
}

template <bool IOU, bool QUALITY>
__global__ __launch_bounds__(256) void det_loss_bwd_kernel(const float* cls, const float* reg, const float* anchors, const float* ann, int N, int A,
                                                           int K, int Mx, int kind, int cls_kind, const short* assign, const float* npos,
                                                           const float* gout /* [2] */, float* dcls, float* dreg, const unsigned char* valid,
                                                           const float* target /* [N][A] or nullptr (QUALITY only) */) {
    static_assert(IOU || !QUALITY, "the quality terms' target is the box's iou");
    // the block's 256 x K probabilities / gradients are one contiguous run in memory: they move through LDS with coalesced 4-byte
    // accesses (a thread walking its own K floats 36 bytes from its neighbour's wrote partial lines: 0.9 TB/s, 91 us per step); every
    // thread of the block reaches both barriers
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
    const float fr = !(lab && p_n > 0.f) ? 0.f : IOU ? gout[1] / (nlab * p_n) : gout[1] / (nlab * 4.f * p_n);
    // (a given assignment keeps its values for an unlabelled image; a stray value counts as ignored here as in the forward, so it never
    // indexes the annotations)
    const int as = a < A && lab ? det_given_assign(assign[(long)n * A + a], Mx) : -2;
    const float* an = ann + (long)n * Mx * 5;
    float g[4] = {0.f, 0.f, 0.f, 0.f};
    float q = 0.f;
    if (as >= 0) {                                                     // the box first: its iou is the quality terms' target
        float loss;
        const float* r = reg + ((long)n * A + a) * 4;
        if (IOU) det_iou_box<true>(r, anchors + (long)a * 4, an + as * 5, kind, loss, q, g);
        else det_smooth_l1<true>(r, anchors + (long)a * 4, an + as * 5, loss, g);
        if (QUALITY && target) q = target[(long)n * A + a];
    }
    if (a < A) {                                                       // (K odd or not: stride-K rows, each thread only touches its own)
        float* c = tile + threadIdx.x * K;
        const int cid = as >= 0 ? (int)an[as * 5 + 4] : -1;
        if (QUALITY) det_quality_grad_row(c, K, as, cid, q, cls_kind, fc);
        else det_focal_grad_row(c, K, as, cid, fc);
    }
    __syncthreads();
    float* dblk = dcls + ((long)n * A + a0) * K;
    for (int i = threadIdx.x; i < nv * K; i += 256) dblk[i] = tile[i];
    if (a >= A) return;
    // (an anchor without a box gets fr * 0 from the IoU terms, -0 under a negative gout[1], and a plain +0 from smooth-L1)
    const float f = IOU || as >= 0 ? fr : 0.f;
    *reinterpret_cast<f32x4*>(dreg + ((long)n * A + a) * 4) = f32x4{f * g[0], f * g[1], f * g[2], f * g[3]};
}

extern "C" int hn_det_loss_blocks(int A) { return (A + 255) / 256; }   // partial rows per image

// The launchers behind every hn_det_loss* entry point.  reg_kind: 0 smooth-L1, 1 giou, 2 diou, 3 ciou; cls_kind: 0 focal, 1 qfl, 2 vfl
// (1, 2 only with reg_kind != 0); valid: the det row of the task masks (nullptr = every image labelled); target: fp32 [N][A], a positive
// anchor's y under cls_kind 1, 2 instead of its box's iou (nullptr = the iou; only the aligned entry points pass one).
// fwd: out[0] = classification loss, out[1] = regression loss[, out[2] = mean IoU of the positives unless reg_kind 0] (batch means of
// per-image means); assign int16 [N][A] (written, or read when assign_given: values outside -2 .. Mx - 1 count as ignored), part fp32
// [N][blocks][3 for reg_kind 0, else 4], npos fp32 [N]
static int det_loss_fwd(const float* cls, const float* reg, const float* anchors, const float* ann, int N, int A, int K, int Mx,
                        int reg_kind, int cls_kind, const unsigned char* valid, int assign_given, void* assign, float* part, float* npos,
                        float* out, hipStream_t st, const float* target = nullptr) {
    HN_CHECK_ARG(cls && reg && anchors && ann && assign && part && npos && out && N > 0 && A > 0 && K > 0 && K <= HN_DET_MAXK && Mx > 0);
    HN_CHECK_ARG(reg_kind >= 0 && reg_kind <= 3 && cls_kind >= 0 && cls_kind <= (reg_kind ? 2 : 0) && (assign_given == 0 || assign_given == 1));
    static void (*const kernels[3][2])(const float*, const float*, const float*, const float*, int, int, int, int, int, short*, float*,
                                       const unsigned char*, const float*) = {
        {det_loss_fwd_kernel<false, false, false>, det_loss_fwd_kernel<false, false, true>},
        {det_loss_fwd_kernel<true, false, false>, det_loss_fwd_kernel<true, false, true>},
        {det_loss_fwd_kernel<true, true, false>, det_loss_fwd_kernel<true, true, true>}};
    const int blocks = hn_det_loss_blocks(A);
    hipLaunchKernelGGL(kernels[!reg_kind ? 0 : !cls_kind ? 1 : 2][assign_given], dim3(blocks, N), dim3(256), 0, st, cls, reg, anchors, ann, A, K,
                       Mx, reg_kind, cls_kind, (short*)assign, part, valid, target);
    if (reg_kind) hipLaunchKernelGGL((det_loss_finalize_kernel<4, 1>), dim3(1), dim3(1024), 0, st, part, blocks, N, npos, out, valid);
    else hipLaunchKernelGGL((det_loss_finalize_kernel<3, 4>), dim3(1), dim3(1024), 0, st, part, blocks, N, npos, out, valid);
    HN_LAUNCH_CHECK();
}

static int det_loss_bwd(const float* cls, const float* reg, const float* anchors, const float* ann, int N, int A, int K, int Mx,
                        int reg_kind, int cls_kind, const unsigned char* valid, const void* assign, const float* npos, const float* gout,
                        float* dcls, float* dreg, hipStream_t st, const float* target = nullptr) {
    HN_CHECK_ARG(cls && reg && anchors && ann && assign && npos && gout && dcls && dreg && N > 0 && A > 0 && K > 0 && Mx > 0);
    HN_CHECK_ARG(K <= HN_DET_MAXK);                                     // 256 x K floats of LDS
    HN_CHECK_ARG(reg_kind >= 0 && reg_kind <= 3 && cls_kind >= 0 && cls_kind <= (reg_kind ? 2 : 0));
    static void (*const kernels[3])(const float*, const float*, const float*, const float*, int, int, int, int, int, int, const short*,
                                    const float*, const float*, float*, float*, const unsigned char*, const float*) = {
        det_loss_bwd_kernel<false, false>, det_loss_bwd_kernel<true, false>, det_loss_bwd_kernel<true, true>};
    hipLaunchKernelGGL(kernels[!reg_kind ? 0 : !cls_kind ? 1 : 2], dim3(hn_det_loss_blocks(A), N), dim3(256), 256 * (size_t)K * sizeof(float), st,
                       cls, reg, anchors, ann, N, A, K, Mx, reg_kind, cls_kind, (const short*)assign, npos, gout, dcls, dreg, valid, target);
    HN_LAUNCH_CHECK();
}

// ---- the exported names (include/hydranet_hip.h): each checks what only it rejects and forwards to a launcher ----
// smooth-L1 + focal
extern "C" int hn_det_loss_fwd(const float* cls, const float* reg, const float* anchors, const float* ann, int N, int A, int K, int Mx,
                               void* assign, float* part, float* npos, float* out, hipStream_t st) {
    return det_loss_fwd(cls, reg, anchors, ann, N, A, K, Mx, 0, 0, nullptr, 0, assign, part, npos, out, st);
}
extern "C" int hn_det_loss_fwd_masked(const float* cls, const float* reg, const float* anchors, const float* ann, int N, int A, int K, int Mx,
                                      const unsigned char* valid, void* assign, float* part, float* npos, float* out, hipStream_t st) {
    HN_CHECK_ARG(valid);
    return det_loss_fwd(cls, reg, anchors, ann, N, A, K, Mx, 0, 0, valid, 0, assign, part, npos, out, st);
}
extern "C" int hn_det_loss_fwd_assigned(const float* cls, const float* reg, const float* anchors, const float* ann, int N, int A, int K, int Mx,
                                        const void* assign, float* part, float* npos, float* out, hipStream_t st) {
    return det_loss_fwd(cls, reg, anchors, ann, N, A, K, Mx, 0, 0, nullptr, 1, (void*)assign, part, npos, out, st);
}
extern "C" int hn_det_loss_fwd_assigned_masked(const float* cls, const float* reg, const float* anchors, const float* ann, int N, int A, int K,
                                               int Mx, const unsigned char* valid, const void* assign, float* part, float* npos, float* out,
                                               hipStream_t st) {
    HN_CHECK_ARG(valid);
    return det_loss_fwd(cls, reg, anchors, ann, N, A, K, Mx, 0, 0, valid, 1, (void*)assign, part, npos, out, st);
}
extern "C" int hn_det_loss_bwd(const float* cls, const float* reg, const float* anchors, const float* ann, int N, int A, int K, int Mx,
                               const void* assign, const float* npos, const float* gout, float* dcls, float* dreg, hipStream_t st) {
    return det_loss_bwd(cls, reg, anchors, ann, N, A, K, Mx, 0, 0, nullptr, assign, npos, gout, dcls, dreg, st);
}
extern "C" int hn_det_loss_bwd_masked(const float* cls, const float* reg, const float* anchors, const float* ann, int N, int A, int K, int Mx,
                                      const unsigned char* valid, const void* assign, const float* npos, const float* gout, float* dcls,
                                      float* dreg, hipStream_t st) {
    HN_CHECK_ARG(valid);
    return det_loss_bwd(cls, reg, anchors, ann, N, A, K, Mx, 0, 0, valid, assign, npos, gout, dcls, dreg, st);
}

// giou / diou / ciou (kind 1..3) + focal
extern "C" int hn_det_loss_iou_fwd(const float* cls, const float* reg, const float* anchors, const float* ann, int N, int A, int K, int Mx,
                                   int kind, void* assign, float* part, float* npos, float* out, hipStream_t st) {
    HN_CHECK_ARG(kind >= 1);
    return det_loss_fwd(cls, reg, anchors, ann, N, A, K, Mx, kind, 0, nullptr, 0, assign, part, npos, out, st);
}
extern "C" int hn_det_loss_iou_fwd_masked(const float* cls, const float* reg, const float* anchors, const float* ann, int N, int A, int K,
                                          int Mx, int kind, const unsigned char* valid, void* assign, float* part, float* npos, float* out,
                                          hipStream_t st) {
    HN_CHECK_ARG(valid && kind >= 1);
    return det_loss_fwd(cls, reg, anchors, ann, N, A, K, Mx, kind, 0, valid, 0, assign, part, npos, out, st);
}
extern "C" int hn_det_loss_iou_fwd_assigned(const float* cls, const float* reg, const float* anchors, const float* ann, int N, int A, int K,
                                            int Mx, int kind, const void* assign, float* part, float* npos, float* out, hipStream_t st) {
    HN_CHECK_ARG(kind >= 1);
    return det_loss_fwd(cls, reg, anchors, ann, N, A, K, Mx, kind, 0, nullptr, 1, (void*)assign, part, npos, out, st);
}
extern "C" int hn_det_loss_iou_fwd_assigned_masked(const float* cls, const float* reg, const float* anchors, const float* ann, int N, int A,
                                                   int K, int Mx, int kind, const unsigned char* valid, const void* assign, float* part,
                                                   float* npos, float* out, hipStream_t st) {
    HN_CHECK_ARG(valid && kind >= 1);
    return det_loss_fwd(cls, reg, anchors, ann, N, A, K, Mx, kind, 0, valid, 1, (void*)assign, part, npos, out, st);
}
extern "C" int hn_det_loss_iou_bwd(const float* cls, const float* reg, const float* anchors, const float* ann, int N, int A, int K, int Mx,
                                   int kind, const void* assign, const float* npos, const float* gout, float* dcls, float* dreg,
                                   hipStream_t st) {
    HN_CHECK_ARG(kind >= 1);
    return det_loss_bwd(cls, reg, anchors, ann, N, A, K, Mx, kind, 0, nullptr, assign, npos, gout, dcls, dreg, st);
}
extern "C" int hn_det_loss_iou_bwd_masked(const float* cls, const float* reg, const float* anchors, const float* ann, int N, int A, int K,
                                          int Mx, int kind, const unsigned char* valid, const void* assign, const float* npos,
                                          const float* gout, float* dcls, float* dreg, hipStream_t st) {
    HN_CHECK_ARG(valid && kind >= 1);
    return det_loss_bwd(cls, reg, anchors, ann, N, A, K, Mx, kind, 0, valid, assign, npos, gout, dcls, dreg, st);
}

// giou / diou / ciou + qfl / vfl (cls_kind 1..2); valid and assign_given are arguments
extern "C" int hn_det_loss_quality_fwd(const float* cls, const float* reg, const float* anchors, const float* ann, int N, int A, int K, int Mx,
                                       int kind, int cls_kind, const unsigned char* valid, int assign_given, void* assign, float* part,
                                       float* npos, float* out, hipStream_t st) {
    HN_CHECK_ARG(kind >= 1 && cls_kind >= 1);
    return det_loss_fwd(cls, reg, anchors, ann, N, A, K, Mx, kind, cls_kind, valid, assign_given, assign, part, npos, out, st);
}
extern "C" int hn_det_loss_quality_bwd(const float* cls, const float* reg, const float* anchors, const float* ann, int N, int A, int K, int Mx,
                                       int kind, int cls_kind, const unsigned char* valid, const void* assign, const float* npos,
                                       const float* gout, float* dcls, float* dreg, hipStream_t st) {
    HN_CHECK_ARG(kind >= 1 && cls_kind >= 1);
    return det_loss_bwd(cls, reg, anchors, ann, N, A, K, Mx, kind, cls_kind, valid, assign, npos, gout, dcls, dreg, st);
}

// the quality pair with the positives' classification target handed in (hn_det_tal_assign's aligned target, read with its assignment):
// y = target[n][a] for a positive anchor in the forward and in the backward; the regression term, out[2], npos and dreg do not read it
extern "C" int hn_det_loss_aligned_fwd(const float* cls, const float* reg, const float* anchors, const float* ann, int N, int A, int K, int Mx,
                                       int kind, int cls_kind, const unsigned char* valid, int assign_given, void* assign, const float* target,
                                       float* part, float* npos, float* out, hipStream_t st) {
    HN_CHECK_ARG(kind >= 1 && cls_kind >= 1 && target && assign_given == 1);     // a target belongs to a given assignment
    return det_loss_fwd(cls, reg, anchors, ann, N, A, K, Mx, kind, cls_kind, valid, 1, assign, part, npos, out, st, target);
}
extern "C" int hn_det_loss_aligned_bwd(const float* cls, const float* reg, const float* anchors, const float* ann, int N, int A, int K, int Mx,
                                       int kind, int cls_kind, const unsigned char* valid, const void* assign, const float* target,
                                       const float* npos, const float* gout, float* dcls, float* dreg, hipStream_t st) {
    HN_CHECK_ARG(kind >= 1 && cls_kind >= 1 && target);
    return det_loss_bwd(cls, reg, anchors, ann, N, A, K, Mx, kind, cls_kind, valid, assign, npos, gout, dcls, dreg, st, target);
}
