// What the detection kernels of more than one source share: the per-image task masks (every masked loss, hn_loss.hip included), the IoU
// anchor assignment (FocalLoss.forward, head_detect/detection_loss.py:132-267; hn_det_atss.hip restates its IoU), the box function of
// the IoU-family terms (the loss's regression term and quality target, hn_det_tal.hip's alignment metric) and the finalize kernel of the
// detection loss.  The loss's other terms and its kernel pair are hn_det_loss.hip's.
#pragma once
#include "hn_common.h"

#define HN_DET_MAXK 32

// Per-image task masks (gt_dict["task_valid"], one uint8 row per task: 1 = image n carries a label for the task).  Every masked entry
// point (hn_*_masked) runs its unmasked twin's kernels with the row handed in; valid == nullptr is the unmasked call.  The number of
// labelled images is counted where it is needed, by the thread that needs it, in image order: N bytes, no extra launch, no atomics.
__device__ __forceinline__ int hn_count_valid(const unsigned char* valid, int N) {
    if (!valid) return N;
    int c = 0;
    for (int n = 0; n < N; ++n) c += valid[n] != 0 ? 1 : 0;
    return c;
}
__device__ __forceinline__ bool hn_image_valid(const unsigned char* valid, int n) { return !valid || valid[n] != 0; }

// assign: >= 0 matched annotation, -1 background, -2 ignored (IoU: neg < 0.4, pos >= 0.5)
__device__ __forceinline__ int det_assign(const float* anc, const float* ann, int Mx, float& best_iou) {
    const float ay1 = anc[0], ax1 = anc[1], ay2 = anc[2], ax2 = anc[3];
    const float aarea = (ay2 - ay1) * (ax2 - ax1);
    float best = -1.f;
    int arg = -1;
    bool any = false;
    for (int j = 0; j < Mx; ++j) {
        const float* b = ann + j * 5;
        if (b[4] == -1.f) continue;
        any = true;
        const float area = (b[2] - b[0]) * (b[3] - b[1]);
        float iw = fminf(ax2, b[2]) - fmaxf(ax1, b[0]);
        float ih = fminf(ay2, b[3]) - fmaxf(ay1, b[1]);
        iw = fmaxf(iw, 0.f);
        ih = fmaxf(ih, 0.f);
        float ua = aarea + area - iw * ih;
        ua = fmaxf(ua, 1e-8f);
        const float iou = iw * ih / ua;
        if (iou > best) { best = iou; arg = j; }                      // first maximum wins, like torch.max
    }
    best_iou = best;
    if (!any) return -1;                                              // image without boxes: every anchor is background
    if (best >= 0.5f) return arg;
    if (best < 0.4f) return -1;
    return -2;
}

// an assignment handed to the loss forward (ATSS, hn_det_atss.hip): anything that is not an annotation index, -1 or -2 counts as ignored,
// so a stray value never indexes the annotations
__device__ __forceinline__ int det_given_assign(short v, int Mx) { return v >= -2 && v < Mx ? (int)v : -2; }

// One block of 1024 threads folds the forward's partial rows part[N][blocks][COLS] = {cls, reg, #pos[, extra]}.  Per image:
// cls = sum_cls / max(npos, 1), reg = sum_reg / (REG_PER_POS npos) and extra = sum_extra / npos (both 0 without positives);
// out[0], out[1][, out[2]] = their batch means; npos kept for the backward.  With a mask an unlabelled image's partial rows are zeros
// (its anchors are all ignored), so its terms add +0 to the sums, and the means are taken over the labelled images (0 without any).
// One wave per image (16 images walked one after the other by a single wave took 30 us of dependent load rounds), images beyond 16 in
// further passes; the batch means are summed in image order by one thread.
template <int COLS, int REG_PER_POS>
__global__ __launch_bounds__(1024) void det_loss_finalize_kernel(const float* part, int blocks, int N, float* npos, float* out /* [COLS - 1] */,
                                                                 const unsigned char* valid) {
    static_assert(COLS == 3 || COLS == 4, "partial rows are {cls, reg, #pos} or {cls, reg, #pos, extra}");
    __shared__ float pc[64], pr[64], px[64];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    float tc = 0.f, tr = 0.f, tx = 0.f;
    for (int n0 = 0; n0 < N; n0 += 16) {
        const int n = n0 + wave;
        float c = 0.f, r = 0.f, p = 0.f, x = 0.f;
        if (n < N)
            for (int b = lane; b < blocks; b += 64) {
                const float* q = part + ((long)n * blocks + b) * COLS;
                c += q[0]; r += q[1]; p += q[2];
                if (COLS == 4) x += q[3];
            }
        c = wave_sum(c); r = wave_sum(r); p = wave_sum(p);
        if (COLS == 4) x = wave_sum(x);
        __syncthreads();
        if (lane == 0 && n < N) {
            npos[n] = p;
            pc[wave] = c / fmaxf(p, 1.f);
            pr[wave] = p > 0.f ? r / ((float)REG_PER_POS * p) : 0.f;
            if (COLS == 4) px[wave] = p > 0.f ? x / p : 0.f;
        }
        __syncthreads();
        if (threadIdx.x == 0)
            for (int k = 0; k < 16 && n0 + k < N; ++k) {
                tc += pc[k]; tr += pr[k];
                if (COLS == 4) tx += px[k];
            }
    }
    if (threadIdx.x == 0) {
        const int nv = hn_count_valid(valid, N);
        if (nv == 0) { tc = 0.f; tr = 0.f; tx = 0.f; }
        const int dn = nv > 0 ? nv : 1;
        out[0] = tc / dn; out[1] = tr / dn;
        if (COLS == 4) out[2] = tx / dn;
    }
}

#define HN_DET_IOU_EPS 1e-7f
#define HN_DET_IOU_CLIP 4.135166556742356f                             // log(1000 / 16)

// The box function of the IoU-family losses: the anchor's decoded prediction against its annotation.  Every instantiation decodes,
// overlaps and differentiates a box with these instructions; the quality terms' target is this function's iou.
// loss and iou of one positive anchor; with GRAD also g[4] = d loss / d (dy, dx, dh, dw).  The gradient goes through the box corners
// (x1, y1, x2, y2): a min / max passes it to the side that wins, w h and (for ciou) v add their direct dependence on the sides.
// exp / atan are the precise ones: a few dozen positives per image pay for them, and the decode must not add error to a loss of ~1e-1.
template <bool GRAD>
__device__ __forceinline__ void det_iou_box(const float* r, const float* anc, const float* b, int kind, float& loss, float& iou, float* g) {
    const float ha = anc[2] - anc[0], wa = anc[3] - anc[1];
    const float cya = 0.5f * (anc[0] + anc[2]), cxa = 0.5f * (anc[1] + anc[3]);
    const float cy = r[0] * ha + cya, cx = r[1] * wa + cxa;
    const float h = expf(fminf(r[2], HN_DET_IOU_CLIP)) * ha, w = expf(fminf(r[3], HN_DET_IOU_CLIP)) * wa;
    const float px1 = cx - 0.5f * w, px2 = cx + 0.5f * w, py1 = cy - 0.5f * h, py2 = cy + 0.5f * h;
    float gw = b[2] - b[0], gh = b[3] - b[1];
    const float gcx = b[0] + 0.5f * gw, gcy = b[1] + 0.5f * gh;
    gw = fmaxf(gw, 1.f);
    gh = fmaxf(gh, 1.f);
    const float tx1 = gcx - 0.5f * gw, tx2 = gcx + 0.5f * gw, ty1 = gcy - 0.5f * gh, ty2 = gcy + 0.5f * gh;
    const float iw = fminf(px2, tx2) - fmaxf(px1, tx1), ih = fminf(py2, ty2) - fmaxf(py1, ty1);
    const float iwc = fmaxf(iw, 0.f), ihc = fmaxf(ih, 0.f);
    const float inter = iwc * ihc;
    const float uni = w * h + gw * gh - inter + HN_DET_IOU_EPS;
    iou = inter / uni;
    const float cw = fmaxf(px2, tx2) - fminf(px1, tx1), ch = fmaxf(py2, ty2) - fminf(py1, ty1);
    // d loss / d {inter, w h (the predicted area), cw, ch, cx, cy, w, h}: the last four are the direct dependences only
    float d_inter = -(uni + inter) / (uni * uni), d_area = inter / (uni * uni);
    float d_cw = 0.f, d_ch = 0.f, d_cx = 0.f, d_cy = 0.f, d_w = 0.f, d_h = 0.f;
    if (kind == 1) {
        const float ac = cw * ch + HN_DET_IOU_EPS;
        loss = 1.f - iou + (ac - uni) / ac;
        if (GRAD) {
            d_inter += 1.f / ac;
            d_area -= 1.f / ac;
            d_cw = uni / (ac * ac) * ch;
            d_ch = uni / (ac * ac) * cw;
        }
    } else {
        const float ex = cx - gcx, ey = cy - gcy;
        const float rho2 = ex * ex + ey * ey;
        const float c2 = cw * cw + ch * ch + HN_DET_IOU_EPS;
        loss = 1.f - iou + rho2 / c2;
        if (GRAD) {
            d_cx = 2.f * ex / c2;
            d_cy = 2.f * ey / c2;
            d_cw = -2.f * rho2 / (c2 * c2) * cw;
            d_ch = -2.f * rho2 / (c2 * c2) * ch;
        }
        if (kind == 3) {
            const float k4 = 0.40528473456935109f;                     // 4 / pi^2
            const float da = atanf(gw / gh) - atanf(w / h);
            const float v = k4 * da * da;
            const float alpha = v / (1.f - iou + v + HN_DET_IOU_EPS);
            loss += alpha * v;
            if (GRAD) {
                const float s = alpha * 2.f * k4 * da / (w * w + h * h);  // d atan(w / h) = (h dw - w dh) / (w^2 + h^2)
                d_w = -s * h;
                d_h = s * w;
            }
        }
    }
    if (GRAD) {
        const float d_iw = iw > 0.f ? d_inter * ihc : 0.f, d_ih = ih > 0.f ? d_inter * iwc : 0.f;
        // iw = min(px2, tx2) - max(px1, tx1), cw = max(px2, tx2) - min(px1, tx1): each corner takes the gradient of the term it decides
        const float g_x2 = (px2 < tx2 ? d_iw : 0.f) + (px2 > tx2 ? d_cw : 0.f);
        const float g_x1 = -(px1 > tx1 ? d_iw : 0.f) - (px1 < tx1 ? d_cw : 0.f);
        const float g_y2 = (py2 < ty2 ? d_ih : 0.f) + (py2 > ty2 ? d_ch : 0.f);
        const float g_y1 = -(py1 > ty1 ? d_ih : 0.f) - (py1 < ty1 ? d_ch : 0.f);
        const float G_cx = g_x1 + g_x2 + d_cx, G_cy = g_y1 + g_y2 + d_cy;
        const float G_w = 0.5f * (g_x2 - g_x1) + d_area * h + d_w, G_h = 0.5f * (g_y2 - g_y1) + d_area * w + d_h;
        g[0] = G_cy * ha;
        g[1] = G_cx * wa;
        g[2] = r[2] <= HN_DET_IOU_CLIP ? G_h * h : 0.f;                 // d h / d dh = h, 0 where the clip is active
        g[3] = r[3] <= HN_DET_IOU_CLIP ? G_w * w : 0.f;
    }
}
