// The anchor-free dense head: FCOSHead (mmdet/models/dense_heads/fcos_head.py over anchor_free_head.py).
//
// The candidates are the cell centres: for level l with stride s, cell (y, x) is the point (x*s + s/2, y*s + s/2), s/2 an
// integer division, exact in fp32.  The head's outputs arrive as TWO fp32 row tensors over all levels (level-major rows,
// level l: batch * h_l * w_l rows), read in place:
//     A (rows, stride_a): the class tower's fused head conv, the C class logits at column cls_off
//     R (rows, stride_r): the box tower's fused head conv, the 4 RAW distances at column reg_off
// and the centerness logit in column ctr_off of A, or of R under centerness_on_reg (ctr_in_r).  layout8_host =
// [stride_a, cls_off, stride_r, reg_off, ctr_in_r, ctr_off, norm_on_bbox, giou].  The per-level `Scale`, the exp / relu
// and the test-time `* stride` (fcos_head.py:152-160) are applied here, by the kernels that consume the raw values.
//
//   fcos_score         : score[row] = max_c(sigmoid(cls_c) * sigmoid(ctr)) (fcos_head.py:396), the maximum over the fp32
//                        PRODUCTS, so equal products tie and brcnn_rpn_topk's ascending-index rule decides.
//   fcos_decode_levels : everything between the top-k and multiclass_nms(score_factors=centerness)
//                        (fcos_head.py:415-463, core/bbox/transforms.py distance2bbox, bbox_nms.py:34-62), one thread per
//                        (image, pick, class): valid = class sigmoid > score_thr -- BEFORE the centerness factor --,
//                        score = class sigmoid * centerness sigmoid, (level, pick, class) slot order.
//   fcos_assign        : _get_target_single (fcos_head.py:546-628), one thread per (image, point), a loop over the
//                        image's ground truths; gt_inds int32, -1 background.
//   fcos_loss_*        : FCOSHead.loss (fcos_head.py:164-261): sigmoid focal loss over every (point, class), the
//                        centerness-weighted IoU-log | GIoU loss and the centerness BCE over the positives, the targets
//                        formed in the kernel.  Block partials (fixed order within a thread, LDS tree) -> one workgroup
//                        (strided sums, LDS tree): no float atomics, the same bits from run to run.
//
// The layout, the geometry, the decode kernel and the loss kernels are row_head.h's, instantiated with FcosTraits.
#include "row_head.h"

namespace {

constexpr float FC_INF = 1e8f;

struct FcosGeom : RowGeom {
    float eps_overlap, eps_loss;
};

// ------------------------------------------------------------------------------------------------------------ test time
__global__ __launch_bounds__(256) void fcos_score_kernel(const float* __restrict__ a, const float* __restrict__ r,
                                                        const RowLayout lay, int C, long long rows,
                                                        float* __restrict__ score) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < rows; i += (long long)gridDim.x * blockDim.x) {
        const float* x = a + (size_t)i * lay.sa + lay.cls_off;
        const float ct = sigmoidf_(*ctr_ptr(lay, a, r, (size_t)i));
        float m = sigmoidf_(x[0]) * ct;
        for (int c = 1; c < C; c++) m = fmaxf(m, sigmoidf_(x[c]) * ct);
        score[i] = m;
    }
}


// ------------------------------------------------------------------------------------------------------------- geometry
__device__ __forceinline__ int level_of_point(const FcosGeom& g, int p) {
    int l = 0;
#pragma unroll
    for (int i = 1; i < BRCNN_MAX_LEVELS; i++)
        if (i < g.L && p >= g.start[i]) l = i;
    return l;
}

struct FcosAssign {
    float lo[BRCNN_MAX_LEVELS], hi[BRCNN_MAX_LEVELS], rad[BRCNN_MAX_LEVELS];
    int center_sampling;
};

__global__ __launch_bounds__(256) void fcos_assign_kernel(const FcosGeom g, const FcosAssign as, const float* __restrict__ gts,
                                                         int* __restrict__ gt_inds) {
    const long long total = (long long)g.B * g.n;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x) {
        const int b = (int)(t / g.n), p = (int)(t - (long long)b * g.n);
        const int l = level_of_point(g, p);
        const int cell = p - g.start[l], st = g.stride[l];
        const float px = (float)((cell % g.w[l]) * st + st / 2), py = (float)((cell / g.w[l]) * st + st / 2);
        const int G = g.gt_off[b + 1] - g.gt_off[b];
        float best = FC_INF;
        int pick = -1;
        for (int j = 0; j < G; j++) {
            const float4 gt = *reinterpret_cast<const float4*>(gts + (size_t)(g.gt_off[b] + j) * 4);
            const float dl = px - gt.x, dt = py - gt.y, dr = gt.z - px, db = gt.w - py;
            bool inside;
            if (as.center_sampling) {
                const float cx = (gt.x + gt.z) / 2.f, cy = (gt.y + gt.w) / 2.f;
                const float xmin = cx - as.rad[l], ymin = cy - as.rad[l], xmax = cx + as.rad[l], ymax = cy + as.rad[l];
                const float bx1 = xmin > gt.x ? xmin : gt.x, by1 = ymin > gt.y ? ymin : gt.y;
                const float bx2 = xmax > gt.z ? gt.z : xmax, by2 = ymax > gt.w ? gt.w : ymax;
                inside = fminf(fminf(px - bx1, py - by1), fminf(bx2 - px, by2 - py)) > 0.f;
            } else {
                inside = fminf(fminf(dl, dt), fminf(dr, db)) > 0.f;
            }
            const float far = fmaxf(fmaxf(dl, dt), fmaxf(dr, db));
            const bool in_range = far >= as.lo[l] && far <= as.hi[l];
            const float area = (gt.z - gt.x) * (gt.w - gt.y);
            if (inside && in_range && area < best) { best = area; pick = j; }      // strict: ties keep the lowest index
        }
        gt_inds[t] = pick;
    }
}

// ----------------------------------------------------------------------------------------------------------------- loss
// what one row of the head outputs is: its level, image, point and, for a positive, its targets
struct Point {
    int l, b, gi;       // gi: index into the packed gts, -1 background
    float px, py, t[4], ctr_t;
};

struct FcosTraits : CenternessTraits<FcosTraits> {
    using Geom = FcosGeom;
    using Decode = RowDecode;
    using Cell = Point;
    static constexpr int PARTIALS = 4;              // the fourth: the number of positives
    static constexpr bool HAS_INVALID = false;

    static __device__ __forceinline__ int grad(const FcosGeom&, int term, int) { return term; }      // g3 (3,)

    // distance2bbox around the cell centre (core/bbox/transforms.py), after the Scale and the exp | relu * stride
    static __device__ __forceinline__ float4 decode_box(const RowDecode& lv, int l, int cell, size_t,
                                                        const float* __restrict__ raw, float sc) {
        const int st = lv.stride[l];
        const float px = (float)((cell % lv.width[l]) * st + st / 2);
        const float py = (float)((cell / lv.width[l]) * st + st / 2);
        float d[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const float v = sc * raw[k];
            d[k] = lv.lay.norm_on_bbox ? fmaxf(v, 0.f) * (float)st : expf(v);
        }
        return make_float4(px - d[0], py - d[1], px + d[2], py + d[3]);
    }

    static __device__ __forceinline__ Point locate(const FcosGeom& g, const int* __restrict__ gt_inds,
                                                   const float* __restrict__ gts, int l, long long r, bool want_targets) {
        Point o;
        const int hw = g.h[l] * g.w[l];
        o.l = l;
        o.b = (int)(r / hw);
        const int cell = (int)(r - (long long)o.b * hw);
        const int gi = gt_inds[(size_t)o.b * g.n + g.start[l] + cell];
        o.gi = (gi >= 0 && gi < g.gt_off[o.b + 1] - g.gt_off[o.b]) ? g.gt_off[o.b] + gi : -1;
        if (want_targets && o.gi >= 0) {
            const int st = g.stride[l];
            o.px = (float)((cell % g.w[l]) * st + st / 2);
            o.py = (float)((cell / g.w[l]) * st + st / 2);
            const float4 gt = *reinterpret_cast<const float4*>(gts + (size_t)o.gi * 4);
            o.t[0] = o.px - gt.x; o.t[1] = o.py - gt.y; o.t[2] = gt.z - o.px; o.t[3] = gt.w - o.py;
            if (g.lay.norm_on_bbox) {
#pragma unroll
                for (int k = 0; k < 4; k++) o.t[k] = o.t[k] / (float)st;
            }
            // centerness_target (fcos_head.py:630-649)
            const float lr = fminf(o.t[0], o.t[2]) / fmaxf(o.t[0], o.t[2]);
            const float tb = fminf(o.t[1], o.t[3]) / fmaxf(o.t[1], o.t[3]);
            o.ctr_t = sqrtf(lr * tb);
        }
        return o;
    }

    // The box term of one positive: loss, and with BWD its derivative w.r.t. the four SCALED raw values (scale * raw).
    // corner_box_loss (head_loss.h) of the two boxes decoded around the point
    template <bool BWD>
    static __device__ __forceinline__ float box_term(const FcosGeom& g, const Point& o, const float* __restrict__ raw,
                                                     float scale, float* __restrict__ dscaled) {
        float d[4], v[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            v[k] = scale * raw[k];
            d[k] = g.lay.norm_on_bbox ? fmaxf(v[k], 0.f) : expf(v[k]);
        }
        const float p1x = o.px - d[0], p1y = o.py - d[1], p2x = o.px + d[2], p2y = o.py + d[3];
        const float t1x = o.px - o.t[0], t1y = o.py - o.t[1], t2x = o.px + o.t[2], t2y = o.py + o.t[3];
        float gp[4];
        const float loss = corner_box_loss<BWD>(g.lay.giou, g.eps_overlap, g.eps_loss, p1x, p1y, p2x, p2y, t1x, t1y, t2x, t2y, gp);
        if (BWD) {
            const float gd[4] = {-gp[0], -gp[1], gp[2], gp[3]};
#pragma unroll
            for (int k = 0; k < 4; k++)
                dscaled[k] = g.lay.norm_on_bbox ? (v[k] > 0.f ? gd[k] : 0.f) : gd[k] * d[k];
        }
        return loss;
    }
};  // FcosTraits

// norm2 = [number of positives of the batch, sum of their centerness targets]
__global__ __launch_bounds__(256) void fcos_loss_norm_kernel(const FcosGeom g, const float* __restrict__ partials,
                                                            float* __restrict__ norm2) {
    __shared__ float red[CH_THREADS];
    const int tid = threadIdx.x;
    const float cnt = term_sum(g, partials, 3, 1, red, tid), sum = term_sum(g, partials, 2, 1, red, tid);
    if (tid == 0) { norm2[0] = cnt; norm2[1] = sum; }
}

// losses3 = [loss_cls, loss_bbox, loss_centerness]; coef3 = [lw_cls / N, lw_bbox / S, lw_ctr / N] for the backward pass
__global__ __launch_bounds__(256) void fcos_loss_finalize_kernel(const FcosGeom g, const float* __restrict__ partials,
                                                                const float* __restrict__ norm2,
                                                                float* __restrict__ losses3, float* __restrict__ coef3) {
    __shared__ float red[CH_THREADS];
    const int tid = threadIdx.x;
    const float cls = term_sum(g, partials, 0, 0, red, tid), box = term_sum(g, partials, 0, 1, red, tid),
                ctr = term_sum(g, partials, 1, 1, red, tid);
    if (tid == 0) {
        const float N = fmaxf(norm2[0], 1.f), S = fmaxf(norm2[1], 1e-6f);
        losses3[0] = g.lw_cls * (cls / N);
        losses3[1] = g.lw_bbox * (box / S);
        losses3[2] = g.lw_ctr * (ctr / N);
        coef3[0] = g.lw_cls / N;
        coef3[1] = g.lw_bbox / S;
        coef3[2] = g.lw_ctr / N;
    }
}

// --------------------------------------------------------------------------------------------------------------- host
// cfg7_host: [focal gamma, focal alpha, eps of bbox_overlaps, eps of the IoU-log clamp, loss_weight_cls, loss_weight_bbox,
// loss_weight_centerness]
int fill_geom(FcosGeom& g, int batch, int num_levels, const int* heights, const int* widths, const int* strides,
              int C, const int* gt_offsets_host, const int* layout8, const float* cfg7) {
    const int st = fill_geom_common(g, batch, num_levels, heights, widths, strides, C, gt_offsets_host, layout8);
    if (st) return st;
    g.eps_overlap = g.eps_loss = 1e-6f;
    if (cfg7) {
        g.gamma = cfg7[0]; g.alpha = cfg7[1]; g.eps_overlap = cfg7[2]; g.eps_loss = cfg7[3];
        g.lw_cls = cfg7[4]; g.lw_bbox = cfg7[5]; g.lw_ctr = cfg7[6];
        if (g.gamma < 0.f || !(g.eps_overlap > 0.f) || !(g.eps_loss > 0.f)) return BRCNN_EINVAL;
    }
    return 0;
}

}  // namespace

BRCNN_API int brcnn_fcos_score(const float* a, const float* r, const int* layout8_host, int num_classes, int64_t rows,
                               float* score, void* stream) {
    if (rows < 0 || num_classes <= 0 || num_classes > 0x7fffff || !layout_ok(layout8_host, num_classes)) return BRCNN_EINVAL;
    if (rows == 0) return 0;
    if (!a || !r || !score) return BRCNN_EINVAL;
    long long g = (rows + 255) / 256;
    if (g > 4096) g = 4096;
    hipLaunchKernelGGL(fcos_score_kernel, dim3((int)g), dim3(256), 0, (hipStream_t)stream, a, r, make_layout(layout8_host),
                       num_classes, (long long)rows, score);
    BRCNN_LAUNCH_CHECK();
    return 0;
}

BRCNN_API int brcnn_fcos_decode_levels(const int64_t* const* topk_inds, const int* counts, const float* a, const float* r,
                                       const int* layout8_host, const float* scales, int batch, int num_levels,
                                       const int* heights, const int* widths, const int* strides, int num_classes,
                                       const float* max_shape, const float* scale_factor, float score_thr, float* boxes,
                                       float* scores, int64_t* labels, uint8_t* valid, int32_t* n_valid, void* stream) {
    RowDecode lv = {};
    const int st = fill_decode_common(lv, topk_inds, counts, a, r, layout8_host, scales, batch, num_levels, heights, widths,
                                      strides, num_classes, max_shape, score_thr, boxes, scores, labels, valid, n_valid);
    if (st) return st;
    return launch_decode_levels<FcosTraits>(lv, batch, a, r, scales, max_shape, scale_factor, boxes, scores, labels, valid,
                                            n_valid, stream);
}

BRCNN_API int brcnn_fcos_assign(const float* gts, const int* gt_offsets_host, int batch, int num_levels, const int* heights,
                                const int* widths, const int* strides, const float* ranges_host, int center_sampling,
                                double center_sample_radius, int32_t* gt_inds, void* stream) {
    FcosGeom g;
    if (!gt_offsets_host || !ranges_host || !gt_inds) return BRCNN_EINVAL;
    const int st = fill_geom(g, batch, num_levels, heights, widths, strides, 1, gt_offsets_host, nullptr, nullptr);
    if (st) return st;
    if (!gts && g.gt_off[batch] > 0) return BRCNN_EINVAL;
    FcosAssign as = {};
    as.center_sampling = center_sampling != 0;
    for (int l = 0; l < num_levels; l++) {
        as.lo[l] = ranges_host[2 * l]; as.hi[l] = ranges_host[2 * l + 1];
        as.rad[l] = (float)((double)strides[l] * center_sample_radius);    // `strides[lvl] * radius` stored into a fp32 tensor
    }
    hipLaunchKernelGGL(fcos_assign_kernel, dim3(rows_grid((long long)batch * g.n)), dim3(256), 0, (hipStream_t)stream, g, as, gts, gt_inds);
    BRCNN_LAUNCH_CHECK();
    return 0;
}

BRCNN_API size_t brcnn_fcos_loss_workspace_bytes(int batch, int num_levels, const int* heights, const int* widths,
                                                 int num_classes) {
    FcosGeom g;
    if (fill_geom(g, batch, num_levels, heights, widths, UnitStrides().v, num_classes, nullptr, nullptr, nullptr)) return 0;
    return loss_workspace_bytes<FcosTraits>(g);
}

BRCNN_API int brcnn_fcos_loss_forward(const float* a, const float* r, const int* layout8_host, const float* scales,
                                      int batch, int num_levels, const int* heights, const int* widths, const int* strides,
                                      int num_classes, const int32_t* gt_inds, const float* gts, const int64_t* gt_labels,
                                      const int* gt_offsets_host, const float* cfg7_host, void* workspace,
                                      size_t workspace_bytes, float* norm2, void* stream) {
    FcosGeom g;
    if (!layout8_host || !cfg7_host || !gt_offsets_host) return BRCNN_EINVAL;
    const int st = fill_geom(g, batch, num_levels, heights, widths, strides, num_classes, gt_offsets_host, layout8_host,
                             cfg7_host);
    if (st) return st;
    if (!a || !r || !scales || !gt_inds || !workspace || !norm2 || ((!gts || !gt_labels) && g.gt_off[batch] > 0) ||
        workspace_bytes < loss_workspace_bytes<FcosTraits>(g))
        return BRCNN_EINVAL;
    float* partials = (float*)workspace;
    const int fs = launch_loss_forward<FcosTraits>(g, ScaledRows{a, r, scales}, gt_inds, gts, gt_labels, partials, stream);
    if (fs) return fs;
    hipLaunchKernelGGL(fcos_loss_norm_kernel, dim3(1), dim3(CH_THREADS), 0, (hipStream_t)stream, g, partials, norm2);
    BRCNN_LAUNCH_CHECK();
    return 0;
}

BRCNN_API int brcnn_fcos_loss_finalize(const void* workspace, size_t workspace_bytes, const float* norm2, int batch,
                                       int num_levels, const int* heights, const int* widths, int num_classes,
                                       const float* cfg7_host, float* losses3, float* coef3, void* stream) {
    FcosGeom g;
    if (!cfg7_host) return BRCNN_EINVAL;
    const int st = fill_geom(g, batch, num_levels, heights, widths, UnitStrides().v, num_classes, nullptr, nullptr, cfg7_host);
    if (st) return st;
    if (!workspace || !norm2 || !losses3 || !coef3 || workspace_bytes < loss_workspace_bytes<FcosTraits>(g))
        return BRCNN_EINVAL;
    hipLaunchKernelGGL(fcos_loss_finalize_kernel, dim3(1), dim3(CH_THREADS), 0, (hipStream_t)stream, g,
                       (const float*)workspace, norm2, losses3, coef3);
    BRCNN_LAUNCH_CHECK();
    return 0;
}

BRCNN_API int brcnn_fcos_loss_backward(const float* a, const float* r, const int* layout8_host, const float* scales,
                                       int batch, int num_levels, const int* heights, const int* widths, const int* strides,
                                       int num_classes, const int32_t* gt_inds, const float* gts, const int64_t* gt_labels,
                                       const int* gt_offsets_host, const float* cfg7_host, const float* grad_losses3,
                                       const float* coef3, void* workspace, size_t workspace_bytes, float* da, float* dr,
                                       float* dscale, void* stream) {
    FcosGeom g;
    if (!layout8_host || !cfg7_host || !gt_offsets_host) return BRCNN_EINVAL;
    const int st = fill_geom(g, batch, num_levels, heights, widths, strides, num_classes, gt_offsets_host, layout8_host,
                             cfg7_host);
    if (st) return st;
    return launch_loss_backward<FcosTraits>(g, a, r, scales, gt_inds, gts, gt_labels, grad_losses3, coef3, workspace,
                                            workspace_bytes, da, dr, dscale, stream);
}
