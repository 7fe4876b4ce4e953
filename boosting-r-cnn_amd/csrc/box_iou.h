// bbox_overlaps for one pair of boxes, shared by the assignment kernels (targets.hip, atss_head.hip).
#pragma once
#include "common.h"

// bbox_overlaps(gt, box) for one pair, the reference's operation order (iou2d_calculator.py:232-261):
// area1 = gt, area2 = box, union = area1 + area2 - overlap, max(union, eps), overlap / union
__device__ __forceinline__ float pair_iou(const float4 g, const float ga, const float4 b, const float ba) {
    const float ltx = fmaxf(g.x, b.x), lty = fmaxf(g.y, b.y);
    const float rbx = fminf(g.z, b.z), rby = fminf(g.w, b.w);
    float w = rbx - ltx, h = rby - lty;
    w = w < 0.f ? 0.f : w;
    h = h < 0.f ? 0.f : h;
    const float ov = w * h;
    float un = ga + ba - ov;
    un = fmaxf(un, 1e-6f);
    return ov / un;
}
