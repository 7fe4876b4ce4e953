// The GFL head: GFLHead (mmdet/models/dense_heads/gfl_head.py) with QualityFocalLoss / DistributionFocalLoss
// (models/losses/gfocal_loss.py), trained on brcnn_atss_assign's gt_inds.
//
// One anchor per cell, regenerated where it is needed (row_head.h: anchor_of); only its centre is used.  The head's
// outputs are two fp32 row tensors: A with the C class logits, R with the 4 * (reg_max + 1) RAW box logits, side-major
// [left | top | right | bottom]; logit = scale_l * raw is formed here.  A side's distance is the expectation of the
// max-subtracted softmax over its reg_max + 1 logits, exp sum and expectation accumulated in bin order.
//
//   gfl_decode_levels : one thread per (image, pick, class) slot; distance * stride from the anchor centre, then
//                       decode_tail.h's store_candidate.  score = sigmoid(cls_c): GFL has no centerness.
//   gfl_loss_*        : GFLHead.loss in the block-partial scheme of row_head.h: fixed order within a thread, LDS tree, one
//                       finalize workgroup; no float atomics, the same bits from run to run.  The class term reads a per-row
//                       quality (the IoU of the row's decoded box, recomputed by the one thread that needs it).  The dR
//                       kernel is this file's own: a box row is 4 * (reg_max + 1) wide with two loss terms on it.
//
// The layout, the geometry, the decode kernel, the loss forward and the dA kernels are row_head.h's, instantiated with GflTraits.
#include "box_iou.h"
#include "row_head.h"

namespace {

constexpr int GFL_MAX_REG = 16;

struct GflGeom : RowGeom {
    float base[BRCNN_MAX_LEVELS][4];
    int reg_max;
    float beta, eps, lw_dfl;
};

struct GflDecode : RowDecode {
    float base[BRCNN_MAX_LEVELS][4];
    int reg_max;
};

// the integral of one side: logits x_i = sc * raw[i], i = 0 .. n.  Returns the expectation sum p_i * i; *mx the maximum,
// *z the sum of exp(x_i - mx)
__device__ __forceinline__ float side_integral(const float* __restrict__ raw, float sc, int n, float* mx, float* z) {
    float m = sc * raw[0];
    for (int i = 1; i <= n; i++) m = fmaxf(m, sc * raw[i]);
    float zs = 0.f;
    for (int i = 0; i <= n; i++) zs += expf(sc * raw[i] - m);
    float d = 0.f;
    for (int i = 0; i <= n; i++) d += (expf(sc * raw[i] - m) / zs) * (float)i;
    *mx = m;
    *z = zs;
    return d;
}

// ------------------------------------------------------------------------------------------------------------------ loss
// what one row of the head outputs is: its image, its state and, for a positive, centre and target in units of the stride
struct GflCell {
    int b, gi;          // gi: index into the packed gts (positive), -1 negative, -2 invalid (weight 0)
    float cx, cy;       // the anchor centre / stride
    float4 gt;          // the ground truth / stride
};

__device__ __forceinline__ GflCell gfl_locate(const GflGeom& g, const int* __restrict__ gt_inds, const float* __restrict__ gts,
                                              int l, long long r, bool want_targets) {
    GflCell o;
    const int hw = g.h[l] * g.w[l];
    o.b = (int)(r / hw);
    const int cell = (int)(r - (long long)o.b * hw);
    const int gi = gt_inds[(size_t)o.b * g.n + g.start[l] + cell];
    o.gi = gi < 0 ? -2 : ((gi > 0 && gi <= g.gt_off[o.b + 1] - g.gt_off[o.b]) ? g.gt_off[o.b] + gi - 1 : -1);
    if (want_targets && o.gi >= 0) {
        const float st = (float)g.stride[l];
        const float4 an = anchor_of(g.base[l], g.w[l], g.stride[l], cell);
        o.cx = ((an.z + an.x) / 2.f) / st;
        o.cy = ((an.w + an.y) / 2.f) / st;
        const float4 gt = *reinterpret_cast<const float4*>(gts + (size_t)o.gi * 4);
        o.gt = make_float4(gt.x / st, gt.y / st, gt.z / st, gt.w / st);
    }
    return o;
}

// the decoded box of a positive row (stride units) and the softmax statistics of its four sides
struct GflBox {
    float d[4], m[4], z[4];
    float4 p;
};

__device__ __forceinline__ GflBox gfl_box(const GflGeom& g, const GflCell& o, const float* __restrict__ raw, float sc) {
    GflBox x;
    const int w = g.reg_max + 1;
#pragma unroll
    for (int k = 0; k < 4; k++) x.d[k] = side_integral(raw + k * w, sc, g.reg_max, &x.m[k], &x.z[k]);
    x.p = make_float4(o.cx - x.d[0], o.cy - x.d[1], o.cx + x.d[2], o.cy + x.d[3]);
    return x;
}

// quality = aligned bbox_overlaps(decoded box, target), eps 1e-6 (iou2d_calculator.py: area1 the prediction's)
__device__ __forceinline__ float gfl_quality(const GflBox& x, const GflCell& o) {
    return pair_iou(x.p, (x.p.z - x.p.x) * (x.p.w - x.p.y), o.gt, (o.gt.z - o.gt.x) * (o.gt.w - o.gt.y));
}

// weight = max_c sigmoid(cls_c) of a row
__device__ __forceinline__ float gfl_weight(const GflGeom& g, const float* __restrict__ a, size_t row) {
    const float* x = a + row * g.lay.sa + g.lay.cls_off;
    float w = sigmoidf_(x[0]);
    for (int c = 1; c < g.C; c++) w = fmaxf(w, sigmoidf_(x[c]));
    return w;
}

// bbox2distance (transforms.py) of side k: the distance from the centre to the target's side, clamped to [0, reg_max - 0.1]
__device__ __forceinline__ float gfl_target_side(const GflGeom& g, const GflCell& o, int k) {
    const float t = k == 0 ? o.cx - o.gt.x : (k == 1 ? o.cy - o.gt.y : (k == 2 ? o.gt.z - o.cx : o.gt.w - o.cy));
    const float hi = (float)((double)g.reg_max - 0.1);
    return fminf(fmaxf(t, 0.f), hi);
}

// quality_focal_loss of one (row, class) element.  Off the label: BCE(x, 0) * sigmoid(x)^beta; at a positive's label (hit):
// BCE(x, q) * |q - sigmoid(x)|^beta.  With BWD the derivative w.r.t. x (q is a constant; abs passes sign(0) = 0)
template <bool BWD>
__device__ __forceinline__ float qfl_elem(float x, bool hit, float q, float beta) {
    const float p = sigmoidf_(x);
    if (!hit) {
        const float ce = softplusf_(x), mod = powf(p, beta);
        if (!BWD) return ce * mod;
        return p * mod + ce * (beta * mod * (1.f - p));
    }
    const float ce = bce_logits(x, q), diff = q - p, ad = fabsf(diff);
    if (!BWD) return ce * powf(ad, beta);
    const float sgn = diff > 0.f ? 1.f : (diff < 0.f ? -1.f : 0.f);
    return (p - q) * powf(ad, beta) + ce * (beta * powf(ad, beta - 1.f) * sgn * (-(p * (1.f - p))));
}

// partials: 3 arrays of `nblk` floats.  A class workgroup writes [QFL sum, 0, 0]; a point workgroup [weighted GIoU sum,
// weighted DFL sum, sum of the weights]
struct GflTraits {
    using Geom = GflGeom;
    using Decode = GflDecode;
    using Rows = ScaledRows;
    using Cell = GflCell;
    static constexpr int PARTIALS = 3;
    static constexpr bool HAS_INVALID = true;
    static constexpr bool HAS_CENTERNESS = false;
    static constexpr bool HAS_QUALITY = true;

    static __device__ __forceinline__ int grad(const GflGeom& g, int term, int l) { return term * g.L + l; }      // gl (3, L)

    // the four integrals * stride around the anchor centre
    static __device__ __forceinline__ float4 decode_box(const GflDecode& lv, int l, int cell, size_t,
                                                        const float* __restrict__ raw, float sc) {
        const float4 an = anchor_of(lv.base[l], lv.width[l], lv.stride[l], cell);
        const float cx = (an.z + an.x) / 2.f, cy = (an.w + an.y) / 2.f;
        const float st = (float)lv.stride[l];
        const int w = lv.reg_max + 1;
        float m, z;
        const float d0 = side_integral(raw, sc, lv.reg_max, &m, &z) * st;
        const float d1 = side_integral(raw + w, sc, lv.reg_max, &m, &z) * st;
        const float d2 = side_integral(raw + 2 * w, sc, lv.reg_max, &m, &z) * st;
        const float d3 = side_integral(raw + 3 * w, sc, lv.reg_max, &m, &z) * st;
        return make_float4(cx - d0, cy - d1, cx + d2, cy + d3);
    }

    static __device__ __forceinline__ GflCell locate(const GflGeom& g, const int* __restrict__ gt_inds,
                                                     const float* __restrict__ gts, int l, long long r, bool want_targets) {
        return gfl_locate(g, gt_inds, gts, l, r, want_targets);
    }

    static __device__ __forceinline__ float quality(const GflGeom& g, const ScaledRows& in, const int* __restrict__ gt_inds,
                                                    const float* __restrict__ gts, int l, long long r, size_t row) {
        const GflCell o = gfl_locate(g, gt_inds, gts, l, r, true);
        return gfl_quality(gfl_box(g, o, in.r + row * g.lay.sr + g.lay.reg_off, in.scales[l]), o);
    }

    template <bool BWD>
    static __device__ __forceinline__ float cls_elem(const GflGeom& g, float x, bool hit, float q) {
        return qfl_elem<BWD>(x, hit, q, g.beta);
    }

    static __device__ __forceinline__ void point_terms(const GflGeom& g, const ScaledRows& in, const GflCell& o, int l,
                                                       size_t row, float* acc) {
        const float sc = in.scales[l];
        const float* raw = in.r + row * g.lay.sr + g.lay.reg_off;
        const GflBox x = gfl_box(g, o, raw, sc);
        const float wt = gfl_weight(g, in.a, row);
        acc[0] += corner_box_loss<false>(true, g.eps, g.eps, x.p.x, x.p.y, x.p.z, x.p.w, o.gt.x, o.gt.y, o.gt.z, o.gt.w,
                                         nullptr) * wt;
        float dfl = 0.f;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const float t = gfl_target_side(g, o, k);
            const int left = (int)t;                                     // t >= 0: the truncation is the floor
            const float wl = (float)(left + 1) - t, wr = t - (float)left;
            const float* rk = raw + k * (g.reg_max + 1);
            const float lz = logf(x.z[k]);
            const float ce_l = -((sc * rk[left] - x.m[k]) - lz), ce_r = -((sc * rk[left + 1] - x.m[k]) - lz);
            dfl += ce_l * wl + ce_r * wr;
        }
        acc[1] += dfl * wt * 0.25f;
        acc[2] += wt;
    }
};  // GflTraits

// losses (3, L) = [loss_cls | loss_bbox | loss_dfl] per level; coef3 = [lw_cls / N, lw_bbox / S, lw_dfl / S]
__global__ __launch_bounds__(256) void gfl_loss_finalize_kernel(const GflGeom g, const float* __restrict__ partials,
                                                               const float* __restrict__ norm2, float* __restrict__ losses,
                                                               float* __restrict__ coef3) {
    __shared__ float red[CH_THREADS];
    const int tid = threadIdx.x;
    const float N = fmaxf(norm2[0], 1.f), S = fmaxf(norm2[1], 1.f);
    for (int l = 0; l < g.L; l++) {
        const float cls = level_sum(g, partials, 0, l, 0, red, tid), box = level_sum(g, partials, 0, l, 1, red, tid),
                    dfl = level_sum(g, partials, 1, l, 1, red, tid);
        if (tid == 0) {
            losses[l] = g.lw_cls * (cls / N);
            losses[g.L + l] = g.lw_bbox * box / S;
            losses[2 * g.L + l] = g.lw_dfl * dfl / S;
        }
    }
    if (tid == 0) {
        coef3[0] = g.lw_cls / N;
        coef3[1] = g.lw_bbox / S;
        coef3[2] = g.lw_dfl / S;
    }
}

// one thread per row of dR (rows, stride_r): the 4 * (reg_max + 1) logit columns of a positive, zeros elsewhere; and per
// workgroup the partial of dscale_l = sum over the level's rows of d(scaled logit) * raw
__global__ __launch_bounds__(256) void gfl_loss_backward_r_kernel(const GflGeom g, const float* __restrict__ a,
                                                                 const float* __restrict__ r,
                                                                 const float* __restrict__ scales,
                                                                 const int* __restrict__ gt_inds,
                                                                 const float* __restrict__ gts,
                                                                 const float* __restrict__ gl,
                                                                 const float* __restrict__ coef3, float* __restrict__ dr,
                                                                 float* __restrict__ dscale_partials) {
    __shared__ float red[CH_THREADS];
    const int blk = blockIdx.x, tid = threadIdx.x;
    int l = 0;
#pragma unroll
    for (int i = 1; i < BRCNN_MAX_LEVELS; i++)
        if (i < g.L && blk >= g.pblk0[i]) l = i;
    const long long rows = (long long)g.B * g.h[l] * g.w[l];
    const long long e0 = (long long)(blk - g.pblk0[l]) * CH_CHUNK;
    const int w = g.reg_max + 1;
    const float sc = scales[l];
    float acc = 0.f;
    for (int j = 0; j < CH_PER_THREAD; j++) {
        const long long e = e0 + (long long)j * CH_THREADS + tid;
        if (e >= rows) break;
        const size_t row = (size_t)(g.row0[l] + e);
        float* out = dr + row * g.lay.sr;
        const GflCell o = gfl_locate(g, gt_inds, gts, l, e, true);
        if (o.gi < 0) {
            for (int ch = 0; ch < g.lay.sr; ch++) out[ch] = 0.f;
            continue;
        }
        const float* raw = r + row * g.lay.sr + g.lay.reg_off;
        const GflBox x = gfl_box(g, o, raw, sc);
        const float wt = gfl_weight(g, a, row);
        float gp[4];
        corner_box_loss<true>(true, g.eps, g.eps, x.p.x, x.p.y, x.p.z, x.p.w, o.gt.x, o.gt.y, o.gt.z, o.gt.w, gp);
        // x1 = cx - d0, y1 = cy - d1, x2 = cx + d2, y2 = cy + d3
        const float gd[4] = {-gp[0], -gp[1], gp[2], gp[3]};
        const float kb = gl[g.L + l] * coef3[1] * wt, kd = gl[2 * g.L + l] * coef3[2] * wt * 0.25f;
        for (int ch = 0; ch < g.lay.reg_off; ch++) out[ch] = 0.f;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const float t = gfl_target_side(g, o, k);
            const int left = (int)t;
            const float wl = (float)(left + 1) - t, wr = t - (float)left;
            const float* rk = raw + k * w;
            float* ok = out + g.lay.reg_off + k * w;
            for (int i = 0; i <= g.reg_max; i++) {
                const float p = expf(sc * rk[i] - x.m[k]) / x.z[k];
                // the expectation's and the two cross entropies' derivatives w.r.t. the scaled logit i
                const float ds = kb * (gd[k] * (p * ((float)i - x.d[k]))) +
                                 kd * (wl * (p - (i == left ? 1.f : 0.f)) + wr * (p - (i == left + 1 ? 1.f : 0.f)));
                acc += ds * rk[i];
                ok[i] = ds * sc;
            }
        }
        for (int ch = g.lay.reg_off + 4 * w; ch < g.lay.sr; ch++) out[ch] = 0.f;
    }
    const float s = block_sum(acc, red, tid);
    if (tid == 0) dscale_partials[blk] = s;
}

// --------------------------------------------------------------------------------------------------------------- host
// layout4 (row_head.h) with 4 * (reg_max + 1) box columns
bool gfl_layout_ok(const int* v, int C, int reg_max) {
    return reg_max >= 1 && reg_max <= GFL_MAX_REG && layout4_ok(v, C, 4 * (reg_max + 1));
}

// cfg5_host: [QFL beta, eps of the GIoU, loss_weight_cls, loss_weight_bbox, loss_weight_dfl]
int fill_geom(GflGeom& g, int batch, int num_levels, const int* heights, const int* widths, const int* strides,
              const float* base, int reg_max, int C, const int* gt_offsets_host, const int* layout4, const float* cfg5) {
    const int st = fill_geom_common(g, batch, num_levels, heights, widths, strides, C, gt_offsets_host, nullptr);
    if (st) return st;
    if (reg_max < 1 || reg_max > GFL_MAX_REG) return BRCNN_EINVAL;
    g.reg_max = reg_max;
    if (layout4) {
        if (!gfl_layout_ok(layout4, C, reg_max)) return BRCNN_EINVAL;
        g.lay = make_layout4(layout4);
    }
    for (int l = 0; l < BRCNN_MAX_LEVELS; l++)
        for (int k = 0; k < 4; k++) g.base[l][k] = (base && l < num_levels) ? base[4 * l + k] : 0.f;
    g.beta = 2.f; g.eps = 1e-6f; g.lw_dfl = 1.f;
    if (cfg5) {
        g.beta = cfg5[0]; g.eps = cfg5[1]; g.lw_cls = cfg5[2]; g.lw_bbox = cfg5[3]; g.lw_dfl = cfg5[4];
        if (!(g.beta >= 1.f) || !(g.eps > 0.f)) return BRCNN_EINVAL;
    }
    return 0;
}

}  // namespace

BRCNN_API int brcnn_gfl_decode_levels(const int64_t* const* topk_inds, const int* counts, const float* a, const float* r,
                                      const int* layout4_host, const float* scales, int batch, int num_levels,
                                      const int* heights, const int* widths, const int* strides,
                                      const float* base_anchors_host, int num_classes, int reg_max, const float* max_shape,
                                      const float* scale_factor, float score_thr, float* boxes, float* scores, int64_t* labels,
                                      uint8_t* valid, int32_t* n_valid, void* stream) {
    if (!a || !r || !scales || !base_anchors_host || !max_shape || !boxes || !scores || !labels || !valid || !n_valid ||
        num_classes <= 0 || !gfl_layout_ok(layout4_host, num_classes, reg_max))
        return BRCNN_EINVAL;
    GflDecode lv = {};
    const int st = fill_decode_picks(lv, topk_inds, counts, batch, num_levels, heights, widths, strides, num_classes, score_thr);
    if (st) return st;
    lv.lay = make_layout4(layout4_host);
    lv.reg_max = reg_max;
    fill_decode_base(lv, base_anchors_host, num_levels);
    return launch_decode_levels<GflTraits>(lv, batch, a, r, scales, max_shape, scale_factor, boxes, scores, labels, valid,
                                           n_valid, stream);
}

BRCNN_API size_t brcnn_gfl_loss_workspace_bytes(int batch, int num_levels, const int* heights, const int* widths,
                                                int num_classes) {
    GflGeom g;
    if (fill_geom(g, batch, num_levels, heights, widths, UnitStrides().v, nullptr, 1, num_classes, nullptr, nullptr, nullptr))
        return 0;
    return loss_workspace_bytes<GflTraits>(g);
}

BRCNN_API int brcnn_gfl_loss_forward(const float* a, const float* r, const int* layout4_host, const float* scales, int batch,
                                     int num_levels, const int* heights, const int* widths, const int* strides,
                                     const float* base_anchors_host, int reg_max, int num_classes, const int32_t* gt_inds,
                                     const float* gts, const int64_t* gt_labels, const int* gt_offsets_host,
                                     const float* cfg5_host, void* workspace, size_t workspace_bytes, float* norm2,
                                     void* stream) {
    GflGeom g;
    if (!layout4_host || !cfg5_host || !gt_offsets_host || !base_anchors_host) return BRCNN_EINVAL;
    const int st = fill_geom(g, batch, num_levels, heights, widths, strides, base_anchors_host, reg_max, num_classes,
                             gt_offsets_host, layout4_host, cfg5_host);
    if (st) return st;
    if (!a || !r || !scales || !gt_inds || !workspace || !norm2 || ((!gts || !gt_labels) && g.gt_off[batch] > 0) ||
        workspace_bytes < loss_workspace_bytes<GflTraits>(g))
        return BRCNN_EINVAL;
    float* partials = (float*)workspace;
    const int fs = launch_loss_forward<GflTraits>(g, ScaledRows{a, r, scales}, gt_inds, gts, gt_labels, partials, stream);
    if (fs) return fs;
    hipLaunchKernelGGL(anchor_loss_norm_kernel<GflTraits>, dim3(1), dim3(CH_THREADS), 0, (hipStream_t)stream, g, gt_inds,
                       partials, norm2);
    BRCNN_LAUNCH_CHECK();
    return 0;
}

BRCNN_API int brcnn_gfl_loss_finalize(const void* workspace, size_t workspace_bytes, const float* norm2, int batch,
                                      int num_levels, const int* heights, const int* widths, int num_classes,
                                      const float* cfg5_host, float* losses, float* coef3, void* stream) {
    GflGeom g;
    if (!cfg5_host) return BRCNN_EINVAL;
    const int st = fill_geom(g, batch, num_levels, heights, widths, UnitStrides().v, nullptr, 1, num_classes, nullptr, nullptr,
                             cfg5_host);
    if (st) return st;
    if (!workspace || !norm2 || !losses || !coef3 || workspace_bytes < loss_workspace_bytes<GflTraits>(g)) return BRCNN_EINVAL;
    hipLaunchKernelGGL(gfl_loss_finalize_kernel, dim3(1), dim3(CH_THREADS), 0, (hipStream_t)stream, g, (const float*)workspace,
                       norm2, losses, coef3);
    BRCNN_LAUNCH_CHECK();
    return 0;
}

BRCNN_API int brcnn_gfl_loss_backward(const float* a, const float* r, const int* layout4_host, const float* scales, int batch,
                                      int num_levels, const int* heights, const int* widths, const int* strides,
                                      const float* base_anchors_host, int reg_max, int num_classes, const int32_t* gt_inds,
                                      const float* gts, const int64_t* gt_labels, const int* gt_offsets_host,
                                      const float* cfg5_host, const float* grad_losses, const float* coef3, void* workspace,
                                      size_t workspace_bytes, float* da, float* dr, float* dscale, void* stream) {
    GflGeom g;
    if (!layout4_host || !cfg5_host || !gt_offsets_host || !base_anchors_host) return BRCNN_EINVAL;
    const int st = fill_geom(g, batch, num_levels, heights, widths, strides, base_anchors_host, reg_max, num_classes,
                             gt_offsets_host, layout4_host, cfg5_host);
    if (st) return st;
    if (!loss_backward_args_ok<GflTraits>(g, a, r, scales, gt_inds, gts, gt_labels, grad_losses, coef3, workspace,
                                          workspace_bytes, da, dr, dscale))
        return BRCNN_EINVAL;
    const int as = launch_loss_backward_a<GflTraits>(g, ScaledRows{a, r, scales}, gt_inds, gts, gt_labels, grad_losses, coef3, da,
                                                     stream);
    if (as) return as;
    float* dsp = (float*)workspace;
    hipLaunchKernelGGL(gfl_loss_backward_r_kernel, dim3(g.pblk0[g.L]), dim3(CH_THREADS), 0, (hipStream_t)stream, g, a, r, scales,
                       gt_inds, gts, grad_losses, coef3, dr, dsp);
    BRCNN_LAUNCH_CHECK();
    hipLaunchKernelGGL(rows_dscale_kernel<GflTraits>, dim3(1), dim3(CH_THREADS), 0, (hipStream_t)stream, g, dsp, dscale);
    BRCNN_LAUNCH_CHECK();
    return 0;
}
