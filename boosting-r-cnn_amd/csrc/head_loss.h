// Loss elements shared by the dense heads on row tensors (fcos_head.hip, atss_head.hip, gfl_head.hip, vfnet_head.hip): one
// definition, so that every head evaluates the same fp32 expressions in the same order.
#pragma once
#include "common.h"
#include <float.h>
#include <math.h>

__device__ __forceinline__ float sigmoidf_(float x) { return 1.f / (1.f + expf(-x)); }

// brcnn_sigmoid_focal_loss_forward / _backward's element (csrc/focal_loss.hip), the same arithmetic
template <bool BWD>
__device__ __forceinline__ float focal_elem(float x, bool is_pos, float gamma, float alpha) {
    const float p = 1.f / (1.f + expf(-x));
    if (!BWD) {
        const float term_p = powf(1.f - p, gamma) * logf(fmaxf(p, FLT_MIN));
        const float term_n = powf(p, gamma) * logf(fmaxf(1.f - p, FLT_MIN));
        return is_pos ? -alpha * term_p : -(1.f - alpha) * term_n;
    } else {
        const float term_p = powf(1.f - p, gamma) * (1.f - p - gamma * p * logf(fmaxf(p, FLT_MIN)));
        const float term_n = powf(p, gamma) * (gamma * (1.f - p) * logf(fmaxf(1.f - p, FLT_MIN)) - p);
        return is_pos ? -alpha * term_p : -(1.f - alpha) * term_n;
    }
}

// binary_cross_entropy_with_logits, one element: (1 - t) * x - log_sigmoid(x)
__device__ __forceinline__ float bce_logits(float x, float t) {
    return (1.f - t) * x - (fminf(x, 0.f) - log1pf(expf(-fabsf(x))));
}

// BCE(x, 0) = softplus(x).  Not bce_logits(x, 0.f): its x - (min(x, 0) - log1p(..)) cancels for x < 0 and leaves an error
// of eps * |x| on a value of exp(x) -- this term runs over every (anchor, class), most of them far below 0
__device__ __forceinline__ float softplusf_(float x) { return fmaxf(x, 0.f) + log1pf(expf(-fabsf(x))); }

// The box loss of one (predicted, target) pair of corner boxes: aligned bbox_overlaps (iou2d_calculator.py:192-261), then
// -log(max(iou, eps_loss)) (iou_loss.py:14-50) or, with giou, 1 - giou (:102-117).  With BWD, gp = d loss / d (p1x, p1y,
// p2x, p2y): the reverse of the chain, a max / min / clamp passing the gradient to the operand it selected.
template <bool BWD>
__device__ __forceinline__ float corner_box_loss(bool giou, float eps_overlap, float eps_loss, float p1x, float p1y, float p2x,
                                                 float p2y, float t1x, float t1y, float t2x, float t2y,
                                                 float* __restrict__ gp) {
    const float pw = p2x - p1x, ph = p2y - p1y;
    const float area1 = pw * ph, area2 = (t2x - t1x) * (t2y - t1y);
    const float i1x = fmaxf(p1x, t1x), i1y = fmaxf(p1y, t1y), i2x = fminf(p2x, t2x), i2y = fminf(p2y, t2y);
    const float iw_raw = i2x - i1x, ih_raw = i2y - i1y;
    const float iw = fmaxf(iw_raw, 0.f), ih = fmaxf(ih_raw, 0.f);
    const float overlap = iw * ih;
    const float union_raw = area1 + area2 - overlap;
    const float uni = fmaxf(union_raw, eps_overlap);
    const float iou = overlap / uni;
    float loss, e1x = 0.f, e1y = 0.f, e2x = 0.f, e2y = 0.f, ew_raw = 0.f, eh_raw = 0.f, ew = 0.f, eh = 0.f, hull_raw = 0.f,
                hull = 1.f;
    if (giou) {
        e1x = fminf(p1x, t1x); e1y = fminf(p1y, t1y); e2x = fmaxf(p2x, t2x); e2y = fmaxf(p2y, t2y);
        ew_raw = e2x - e1x; eh_raw = e2y - e1y;
        ew = fmaxf(ew_raw, 0.f); eh = fmaxf(eh_raw, 0.f);
        hull_raw = ew * eh;
        hull = fmaxf(hull_raw, eps_overlap);
        loss = 1.f - (iou - (hull - uni) / hull);
    } else {
        loss = -logf(fmaxf(iou, eps_loss));
    }
    if (BWD) {
        float g_iou, g_uni = 0.f, g_hull = 0.f;
        if (giou) {
            g_iou = -1.f;
            g_uni = -1.f / hull;                             // d(loss)/d(uni) through (hull - uni) / hull
            g_hull = uni / (hull * hull);                     // d(loss)/d(hull): loss = 1 - iou + 1 - uni / hull
        } else {
            g_iou = iou > eps_loss ? -1.f / iou : 0.f;
        }
        float g_overlap = g_iou / uni;
        g_uni += -g_iou * overlap / (uni * uni);
        const float g_union_raw = union_raw > eps_overlap ? g_uni : 0.f;
        const float g_area1 = g_union_raw;
        g_overlap -= g_union_raw;
        const float g_iw = iw_raw >= 0.f ? g_overlap * ih : 0.f, g_ih = ih_raw >= 0.f ? g_overlap * iw : 0.f;
        float g1x = -(g_area1 * ph), g2x = g_area1 * ph, g1y = -(g_area1 * pw), g2y = g_area1 * pw;
        if (p2x < t2x) g2x += g_iw; else if (p2x == t2x) g2x += 0.5f * g_iw;
        if (p1x > t1x) g1x -= g_iw; else if (p1x == t1x) g1x -= 0.5f * g_iw;
        if (p2y < t2y) g2y += g_ih; else if (p2y == t2y) g2y += 0.5f * g_ih;
        if (p1y > t1y) g1y -= g_ih; else if (p1y == t1y) g1y -= 0.5f * g_ih;
        if (giou) {
            const float g_hull_raw = hull_raw > eps_overlap ? g_hull : 0.f;
            const float g_ew = ew_raw >= 0.f ? g_hull_raw * eh : 0.f, g_eh = eh_raw >= 0.f ? g_hull_raw * ew : 0.f;
            if (p2x > t2x) g2x += g_ew; else if (p2x == t2x) g2x += 0.5f * g_ew;
            if (p1x < t1x) g1x -= g_ew; else if (p1x == t1x) g1x -= 0.5f * g_ew;
            if (p2y > t2y) g2y += g_eh; else if (p2y == t2y) g2y += 0.5f * g_eh;
            if (p1y < t1y) g1y -= g_eh; else if (p1y == t1y) g1y -= 0.5f * g_eh;
        }
        gp[0] = g1x; gp[1] = g1y; gp[2] = g2x; gp[3] = g2y;
    }
    return loss;
}
