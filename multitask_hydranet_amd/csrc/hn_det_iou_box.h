// The box function of the IoU-family detection losses: one positive anchor's decoded prediction against its annotation.  hn_det_iou.hip
// (focal classification) and hn_det_quality.hip (quality focal / varifocal classification, whose target is this function's iou) both
// build their kernels from it, so the two paths decode, overlap and differentiate a box with the same instructions.  The definition is
// stated at the top of hn_det_iou.hip.
#pragma once
#include "hn_common.h"

#define HN_DET_IOU_EPS 1e-7f
#define HN_DET_IOU_CLIP 4.135166556742356f                             // log(1000 / 16)

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
