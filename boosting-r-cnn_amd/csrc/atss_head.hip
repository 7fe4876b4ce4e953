// The ATSS head: ATSSHead (mmdet/models/dense_heads/atss_head.py) with ATSSAssigner (core/bbox/assigners/atss_assigner.py).
//
// One anchor per cell, regenerated where it is needed: level l, cell (y, x) -> base_l + (x*s, y*s, x*s, y*s), exact in fp32.
// The head's outputs are FCOSHead's two fp32 row tensors (fcos_head.hip): A with the C class logits, R with the 4 RAW
// deltas, the centerness logit where layout8 puts it; delta = scale_l * raw is formed here.
//
//   atss_assign        : one workgroup per (image, ground truth).  Per level, k = min(topk, valid cells) rounds; a round is
//                        a scan of the level's valid cells for the smallest key (distance bits << 32 | cell) above the
//                        previous round's, an LDS tree minimum: distances rank ascending, equal distances by ascending
//                        cell index.  The (L * topk) candidates stay in LDS; thread 0 forms mean + std in (level, rank)
//                        order; every positive candidate claims its anchor with an integer atomic max on
//                        (IoU bits << 32 | ~gt index).  A second launch turns the keys into gt_inds / max_overlaps.
//   atss_decode_levels : rows_decode_levels_kernel with the anchor decode of dense_decode_levels_kernel.
//   atss_loss_*        : ATSSHead.loss, the block-partial scheme of fcos_loss_* (fixed order within a thread, LDS tree, one
//                        finalize workgroup): no float atomics, the same bits from run to run.
//
// The layout, the geometry, the decode kernel and the loss kernels are row_head.h's, instantiated with AtssTraits.
#include "box_iou.h"
#include "row_head.h"

namespace {

constexpr int AT_MAX_TOPK = 16;

struct AtssGeom : RowGeom {
    float base[BRCNN_MAX_LEVELS][4];
    float eps, mean[4], std[4], max_ratio;
};

struct AtssDecode : RowDecode {
    float base[BRCNN_MAX_LEVELS][4];
    float mean[4], std[4], max_ratio;
};

// delta2bbox (delta_xywh_bbox_coder.py:144-237) of one anchor, brcnn_dense_decode_levels' operation order, before the clip
// to the image.  d: the four deltas (scale * raw, or a target).  With GRAD, jac = [d x / d d0, d y / d d1, d w / d d2,
// d h / d d3] of centre and size (the size's is 0 where the wh_ratio_clip clamp is active)
template <bool GRAD>
__device__ __forceinline__ float4 decode_anchor(const float4 an, const float* d, const float* mean, const float* std,
                                                float max_ratio, float* jac) {
    const float dx = d[0] * std[0] + mean[0];
    const float dy = d[1] * std[1] + mean[1];
    const float dw_raw = d[2] * std[2] + mean[2];
    const float dh_raw = d[3] * std[3] + mean[3];
    const float px = (an.x + an.z) * 0.5f, py = (an.y + an.w) * 0.5f;
    const float pw = an.z - an.x, ph = an.w - an.y;
    const float dxw = pw * dx, dyh = ph * dy;
    const float dw = fminf(fmaxf(dw_raw, -max_ratio), max_ratio);
    const float dh = fminf(fmaxf(dh_raw, -max_ratio), max_ratio);
    const float gw = pw * expf(dw), gh = ph * expf(dh);
    const float gx = px + dxw, gy = py + dyh;
    if (GRAD) {
        jac[0] = pw * std[0];
        jac[1] = ph * std[1];
        jac[2] = (dw_raw < -max_ratio || dw_raw > max_ratio) ? 0.f : gw * std[2];
        jac[3] = (dh_raw < -max_ratio || dh_raw > max_ratio) ? 0.f : gh * std[3];
    }
    return make_float4(gx - gw * 0.5f, gy - gh * 0.5f, gx + gw * 0.5f, gy + gh * 0.5f);
}

// ----------------------------------------------------------------------------------------------------------- assignment
struct AtssAssign {
    int topk;
    const int* valid_hw;        // (B, L, 2) or NULL
};

__device__ __forceinline__ unsigned long long block_min(unsigned long long v, unsigned long long* red, int tid) {
    __syncthreads();
    red[tid] = v;
    __syncthreads();
    for (int d = CH_THREADS / 2; d > 0; d >>= 1) {
        if (tid < d && red[tid + d] < red[tid]) red[tid] = red[tid + d];
        __syncthreads();
    }
    return red[0];
}

__global__ __launch_bounds__(256) void atss_assign_kernel(const AtssGeom g, const AtssAssign as, const float* __restrict__ gts,
                                                         unsigned long long* __restrict__ keys) {
    __shared__ unsigned long long red[CH_THREADS];
    __shared__ int cand[BRCNN_MAX_LEVELS * AT_MAX_TOPK];          // anchor index within the image
    __shared__ float cand_iou[BRCNN_MAX_LEVELS * AT_MAX_TOPK];
    __shared__ float cand_side[BRCNN_MAX_LEVELS * AT_MAX_TOPK];   // min(cx - x1, cy - y1, x2 - cx, y2 - cy)
    __shared__ float s_thr;
    const int tid = threadIdx.x, gi = blockIdx.x;
    int b = 0;
    for (int i = 1; i < g.B; i++)
        if (gi >= g.gt_off[i]) b = i;
    const int j = gi - g.gt_off[b];
    const float4 gt = *reinterpret_cast<const float4*>(gts + (size_t)gi * 4);
    const float gcx = (gt.x + gt.z) / 2.f, gcy = (gt.y + gt.w) / 2.f;
    const float garea = (gt.z - gt.x) * (gt.w - gt.y);
    int m = 0;                                                    // candidates so far (uniform over the workgroup)
    for (int l = 0; l < g.L; l++) {
        const int hw = g.h[l] * g.w[l];
        int vh = g.h[l], vw = g.w[l];
        if (as.valid_hw) {
            const int* v = as.valid_hw + ((size_t)b * g.L + l) * 2;
            vh = min(max(v[0], 0), vh);
            vw = min(max(v[1], 0), vw);
        }
        const int k = min(as.topk, vh * vw);
        unsigned long long prev = 0ull;
        for (int rank = 0; rank < k; rank++) {
            unsigned long long best = ~0ull;
            for (int cell = tid; cell < hw; cell += CH_THREADS) {
                if (cell / g.w[l] >= vh || cell % g.w[l] >= vw) continue;
                const float4 an = anchor_of(g.base[l], g.w[l], g.stride[l], cell);
                const float dx = (an.x + an.z) / 2.f - gcx, dy = (an.y + an.w) / 2.f - gcy;
                const float dist = sqrtf(dx * dx + dy * dy);
                const unsigned long long key = ((unsigned long long)__float_as_uint(dist) << 32) | (unsigned)cell;
                if ((rank == 0 || key > prev) && key < best) best = key;
            }
            prev = block_min(best, red, tid);
            if (tid == 0) cand[m + rank] = g.start[l] + min((int)(unsigned)(prev & 0x7fffffffull), hw - 1);   // (a scanned cell)
        }
        m += k;
    }
    __syncthreads();
    for (int c = tid; c < m; c += CH_THREADS) {
        const int idx = cand[c];
        int l = 0;
#pragma unroll
        for (int i = 1; i < BRCNN_MAX_LEVELS; i++)
            if (i < g.L && idx >= g.start[i]) l = i;
        const float4 an = anchor_of(g.base[l], g.w[l], g.stride[l], idx - g.start[l]);
        cand_iou[c] = pair_iou(gt, garea, an, (an.z - an.x) * (an.w - an.y));
        const float cx = (an.x + an.z) / 2.f, cy = (an.y + an.w) / 2.f;
        cand_side[c] = fminf(fminf(cx - gt.x, cy - gt.y), fminf(gt.z - cx, gt.w - cy));
    }
    __syncthreads();
    if (tid == 0) {
        // mean + unbiased std, sequential in (level, rank) order; m == 1 gives 0 / 0 = NaN: no positive
        float sum = 0.f;
        for (int c = 0; c < m; c++) sum += cand_iou[c];
        const float mean = sum / (float)m;
        float ss = 0.f;
        for (int c = 0; c < m; c++) {
            const float d = cand_iou[c] - mean;
            ss += d * d;
        }
        s_thr = mean + sqrtf(ss / (float)(m - 1));
    }
    __syncthreads();
    const float thr = s_thr;
    for (int c = tid; c < m; c += CH_THREADS) {
        if (cand_iou[c] >= thr && cand_side[c] > 0.01f) {
            const unsigned long long key = ((unsigned long long)__float_as_uint(cand_iou[c]) << 32) | (0xffffffffu - (unsigned)j);
            atomicMax(keys + (size_t)b * g.n + cand[c], key);
        }
    }
}

__global__ __launch_bounds__(256) void atss_assign_write_kernel(const AtssGeom g, const AtssAssign as,
                                                               const unsigned long long* __restrict__ keys,
                                                               int* __restrict__ gt_inds, float* __restrict__ max_overlaps) {
    const long long total = (long long)g.B * g.n;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x) {
        const int b = (int)(t / g.n), p = (int)(t - (long long)b * g.n);
        int l = 0;
#pragma unroll
        for (int i = 1; i < BRCNN_MAX_LEVELS; i++)
            if (i < g.L && p >= g.start[i]) l = i;
        const int cell = p - g.start[l];
        bool ok = true;
        if (as.valid_hw) {
            const int* v = as.valid_hw + ((size_t)b * g.L + l) * 2;
            ok = cell / g.w[l] < v[0] && cell % g.w[l] < v[1];
        }
        const unsigned long long key = keys[t];
        const bool pos = ok && key != 0ull;
        gt_inds[t] = !ok ? -1 : (pos ? (int)(0xffffffffu - (unsigned)(key & 0xffffffffull)) + 1 : 0);
        if (max_overlaps) max_overlaps[t] = pos ? __uint_as_float((unsigned)(key >> 32)) : -1e8f;
    }
}

// ------------------------------------------------------------------------------------------------- test time and loss
// what one row of the head outputs is: its image, its state and, for a positive, its anchor and targets
struct AnchorCell {
    int b, gi;          // gi: index into the packed gts (positive), -1 negative, -2 invalid (weight 0)
    float4 an, gt;      // the anchor; gt' = delta2bbox(anchor, bbox2delta(anchor, gt))
    float ctr_t;
};

struct AtssTraits : CenternessTraits<AtssTraits> {
    using Geom = AtssGeom;
    using Decode = AtssDecode;
    using Cell = AnchorCell;
    static constexpr int PARTIALS = 3;              // the positives are counted from gt_inds, per image
    static constexpr bool HAS_INVALID = true;

    static __device__ __forceinline__ int grad(const AtssGeom& g, int term, int l) { return term * g.L + l; }     // gl (3, L)

    // delta2bbox of the cell's anchor, after the Scale
    static __device__ __forceinline__ float4 decode_box(const AtssDecode& lv, int l, int cell, size_t,
                                                        const float* __restrict__ raw, float sc) {
        const float4 an = anchor_of(lv.base[l], lv.width[l], lv.stride[l], cell);
        const float d[4] = {sc * raw[0], sc * raw[1], sc * raw[2], sc * raw[3]};
        return decode_anchor<false>(an, d, lv.mean, lv.std, lv.max_ratio, nullptr);
    }

    static __device__ __forceinline__ AnchorCell locate(const AtssGeom& g, const int* __restrict__ gt_inds,
                                                        const float* __restrict__ gts, int l, long long r, bool want_targets) {
        AnchorCell o;
        const int hw = g.h[l] * g.w[l];
        o.b = (int)(r / hw);
        const int cell = (int)(r - (long long)o.b * hw);
        const int gi = gt_inds[(size_t)o.b * g.n + g.start[l] + cell];
        o.gi = gi < 0 ? -2 : ((gi > 0 && gi <= g.gt_off[o.b + 1] - g.gt_off[o.b]) ? g.gt_off[o.b] + gi - 1 : -1);
        if (want_targets && o.gi >= 0) {
            o.an = anchor_of(g.base[l], g.w[l], g.stride[l], cell);
            const float4 gt = *reinterpret_cast<const float4*>(gts + (size_t)o.gi * 4);
            // bbox2delta (delta_xywh_bbox_coder.py:99-141)
            const float pw = o.an.z - o.an.x, ph = o.an.w - o.an.y;
            float t[4];
            t[0] = ((gt.x + gt.z) * 0.5f - (o.an.x + o.an.z) * 0.5f) / pw;
            t[1] = ((gt.y + gt.w) * 0.5f - (o.an.y + o.an.w) * 0.5f) / ph;
            t[2] = logf((gt.z - gt.x) / pw);
            t[3] = logf((gt.w - gt.y) / ph);
#pragma unroll
            for (int k = 0; k < 4; k++) t[k] = (t[k] - g.mean[k]) / g.std[k];
            o.gt = decode_anchor<false>(o.an, t, g.mean, g.std, g.max_ratio, nullptr);
            // centerness_target (atss_head.py:294-310)
            const float cx = (o.an.z + o.an.x) / 2.f, cy = (o.an.w + o.an.y) / 2.f;
            const float l_ = cx - o.gt.x, t_ = cy - o.gt.y, r_ = o.gt.z - cx, b_ = o.gt.w - cy;
            o.ctr_t = sqrtf((fminf(l_, r_) / fmaxf(l_, r_)) * (fminf(t_, b_) / fmaxf(t_, b_)));
        }
        return o;
    }

    // The box term of one positive: 1 - giou(delta2bbox(anchor, scale * raw), gt'), and with BWD its derivative w.r.t. the four
    // SCALED raw values
    template <bool BWD>
    static __device__ __forceinline__ float box_term(const AtssGeom& g, const AnchorCell& o, const float* __restrict__ raw,
                                                     float scale, float* __restrict__ dscaled) {
        const float d[4] = {scale * raw[0], scale * raw[1], scale * raw[2], scale * raw[3]};
        float jac[4], gp[4];
        const float4 p = decode_anchor<BWD>(o.an, d, g.mean, g.std, g.max_ratio, jac);
        const float loss = corner_box_loss<BWD>(true, g.eps, g.eps, p.x, p.y, p.z, p.w, o.gt.x, o.gt.y, o.gt.z, o.gt.w, gp);
        if (BWD) {
            // x1 = gx - gw / 2, x2 = gx + gw / 2
            dscaled[0] = (gp[0] + gp[2]) * jac[0];
            dscaled[1] = (gp[1] + gp[3]) * jac[1];
            dscaled[2] = (gp[2] - gp[0]) * 0.5f * jac[2];
            dscaled[3] = (gp[3] - gp[1]) * 0.5f * jac[3];
        }
        return loss;
    }
};  // AtssTraits

// losses (3, L) = [loss_cls | loss_bbox | loss_centerness] per level; coef3 = [lw_cls / N, lw_bbox / S, lw_ctr / N]
__global__ __launch_bounds__(256) void atss_loss_finalize_kernel(const AtssGeom g, const float* __restrict__ partials,
                                                                const float* __restrict__ norm2,
                                                                float* __restrict__ losses, float* __restrict__ coef3) {
    __shared__ float red[CH_THREADS];
    const int tid = threadIdx.x;
    const float N = fmaxf(norm2[0], 1.f), S = fmaxf(norm2[1], 1.f);
    for (int l = 0; l < g.L; l++) {
        const float cls = level_sum(g, partials, 0, l, 0, red, tid), box = level_sum(g, partials, 0, l, 1, red, tid),
                    ctr = level_sum(g, partials, 1, l, 1, red, tid);
        if (tid == 0) {
            losses[l] = g.lw_cls * (cls / N);
            losses[g.L + l] = g.lw_bbox * box / S;
            losses[2 * g.L + l] = g.lw_ctr * (ctr / N);
        }
    }
    if (tid == 0) {
        coef3[0] = g.lw_cls / N;
        coef3[1] = g.lw_bbox / S;
        coef3[2] = g.lw_ctr / N;
    }
}

// --------------------------------------------------------------------------------------------------------------- host
// cfg15_host: [focal gamma, focal alpha, eps of the GIoU, loss_weight_cls, loss_weight_bbox, loss_weight_centerness,
// means (4), stds (4), |log(wh_ratio_clip)|]
int fill_geom(AtssGeom& g, int batch, int num_levels, const int* heights, const int* widths, const int* strides,
              const float* base, int C, const int* gt_offsets_host, const int* layout8, const float* cfg15) {
    const int st = fill_geom_common(g, batch, num_levels, heights, widths, strides, C, gt_offsets_host, layout8);
    if (st) return st;
    for (int l = 0; l < BRCNN_MAX_LEVELS; l++)
        for (int k = 0; k < 4; k++) g.base[l][k] = (base && l < num_levels) ? base[4 * l + k] : 0.f;
    g.eps = 1e-6f; g.max_ratio = 0.f;
    for (int k = 0; k < 4; k++) { g.mean[k] = 0.f; g.std[k] = 1.f; }
    if (cfg15) {
        g.gamma = cfg15[0]; g.alpha = cfg15[1]; g.eps = cfg15[2];
        g.lw_cls = cfg15[3]; g.lw_bbox = cfg15[4]; g.lw_ctr = cfg15[5];
        for (int k = 0; k < 4; k++) { g.mean[k] = cfg15[6 + k]; g.std[k] = cfg15[10 + k]; }
        if (g.gamma < 0.f || !(g.eps > 0.f) || !(cfg15[14] > 0.f)) return BRCNN_EINVAL;
        for (int k = 0; k < 4; k++)
            if (!(g.std[k] > 0.f)) return BRCNN_EINVAL;
        g.max_ratio = cfg15[14];
    }
    return 0;
}

}  // namespace

BRCNN_API int brcnn_atss_assign(const float* gts, const int* gt_offsets_host, int batch, int num_levels, const int* heights,
                                const int* widths, const int* strides, const float* base_anchors_host,
                                const int32_t* valid_hw, int topk, void* workspace, size_t workspace_bytes, int32_t* gt_inds,
                                float* max_overlaps, void* stream) {
    AtssGeom g;
    if (!gt_offsets_host || !base_anchors_host || !gt_inds || !workspace || topk <= 0 || topk > AT_MAX_TOPK) return BRCNN_EINVAL;
    const int st = fill_geom(g, batch, num_levels, heights, widths, strides, base_anchors_host, 1, gt_offsets_host, nullptr,
                             nullptr);
    if (st) return st;
    const int total_gt = g.gt_off[batch];
    const size_t need = (size_t)batch * (size_t)g.n * sizeof(unsigned long long);
    if ((!gts && total_gt > 0) || workspace_bytes < need) return BRCNN_EINVAL;
    AtssAssign as = {};
    as.topk = topk;
    as.valid_hw = valid_hw;
    unsigned long long* keys = (unsigned long long*)workspace;
    BRCNN_HIP_CHECK(hipMemsetAsync(keys, 0, need, (hipStream_t)stream));
    if (total_gt > 0) {
        hipLaunchKernelGGL(atss_assign_kernel, dim3(total_gt), dim3(CH_THREADS), 0, (hipStream_t)stream, g, as, gts, keys);
        BRCNN_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(atss_assign_write_kernel, dim3(rows_grid((long long)batch * g.n)), dim3(256), 0, (hipStream_t)stream, g, as, keys, gt_inds,
                       max_overlaps);
    BRCNN_LAUNCH_CHECK();
    return 0;
}

BRCNN_API int brcnn_atss_decode_levels(const int64_t* const* topk_inds, const int* counts, const float* a, const float* r,
                                       const int* layout8_host, const float* scales, int batch, int num_levels,
                                       const int* heights, const int* widths, const int* strides,
                                       const float* base_anchors_host, int num_classes, const float* max_shape,
                                       const float* scale_factor, const float* means4_host, const float* stds4_host,
                                       double wh_ratio_clip, float score_thr, float* boxes, float* scores, int64_t* labels,
                                       uint8_t* valid, int32_t* n_valid, void* stream) {
    if (!base_anchors_host || !means4_host || !stds4_host || !(wh_ratio_clip > 0.0)) return BRCNN_EINVAL;
    AtssDecode lv = {};
    const int st = fill_decode_common(lv, topk_inds, counts, a, r, layout8_host, scales, batch, num_levels, heights, widths,
                                      strides, num_classes, max_shape, score_thr, boxes, scores, labels, valid, n_valid);
    if (st) return st;
    fill_decode_base(lv, base_anchors_host, num_levels);
    for (int k = 0; k < 4; k++) { lv.mean[k] = means4_host[k]; lv.std[k] = stds4_host[k]; }
    lv.max_ratio = (float)fabs(log(wh_ratio_clip));
    return launch_decode_levels<AtssTraits>(lv, batch, a, r, scales, max_shape, scale_factor, boxes, scores, labels, valid,
                                            n_valid, stream);
}

BRCNN_API size_t brcnn_atss_loss_workspace_bytes(int batch, int num_levels, const int* heights, const int* widths,
                                                 int num_classes) {
    AtssGeom g;
    if (fill_geom(g, batch, num_levels, heights, widths, UnitStrides().v, nullptr, num_classes, nullptr, nullptr, nullptr)) return 0;
    return loss_workspace_bytes<AtssTraits>(g);
}

BRCNN_API int brcnn_atss_loss_forward(const float* a, const float* r, const int* layout8_host, const float* scales,
                                      int batch, int num_levels, const int* heights, const int* widths, const int* strides,
                                      const float* base_anchors_host, int num_classes, const int32_t* gt_inds,
                                      const float* gts, const int64_t* gt_labels, const int* gt_offsets_host,
                                      const float* cfg15_host, void* workspace, size_t workspace_bytes, float* norm2,
                                      void* stream) {
    AtssGeom g;
    if (!layout8_host || !cfg15_host || !gt_offsets_host || !base_anchors_host) return BRCNN_EINVAL;
    const int st = fill_geom(g, batch, num_levels, heights, widths, strides, base_anchors_host, num_classes, gt_offsets_host,
                             layout8_host, cfg15_host);
    if (st) return st;
    if (!a || !r || !scales || !gt_inds || !workspace || !norm2 || ((!gts || !gt_labels) && g.gt_off[batch] > 0) ||
        workspace_bytes < loss_workspace_bytes<AtssTraits>(g))
        return BRCNN_EINVAL;
    float* partials = (float*)workspace;
    const int fs = launch_loss_forward<AtssTraits>(g, ScaledRows{a, r, scales}, gt_inds, gts, gt_labels, partials, stream);
    if (fs) return fs;
    hipLaunchKernelGGL(anchor_loss_norm_kernel<AtssTraits>, dim3(1), dim3(CH_THREADS), 0, (hipStream_t)stream, g, gt_inds, partials, norm2);
    BRCNN_LAUNCH_CHECK();
    return 0;
}

BRCNN_API int brcnn_atss_loss_finalize(const void* workspace, size_t workspace_bytes, const float* norm2, int batch,
                                       int num_levels, const int* heights, const int* widths, int num_classes,
                                       const float* cfg15_host, float* losses, float* coef3, void* stream) {
    AtssGeom g;
    if (!cfg15_host) return BRCNN_EINVAL;
    const int st = fill_geom(g, batch, num_levels, heights, widths, UnitStrides().v, nullptr, num_classes, nullptr, nullptr,
                             cfg15_host);
    if (st) return st;
    if (!workspace || !norm2 || !losses || !coef3 || workspace_bytes < loss_workspace_bytes<AtssTraits>(g)) return BRCNN_EINVAL;
    hipLaunchKernelGGL(atss_loss_finalize_kernel, dim3(1), dim3(CH_THREADS), 0, (hipStream_t)stream, g,
                       (const float*)workspace, norm2, losses, coef3);
    BRCNN_LAUNCH_CHECK();
    return 0;
}

BRCNN_API int brcnn_atss_loss_backward(const float* a, const float* r, const int* layout8_host, const float* scales,
                                       int batch, int num_levels, const int* heights, const int* widths, const int* strides,
                                       const float* base_anchors_host, int num_classes, const int32_t* gt_inds,
                                       const float* gts, const int64_t* gt_labels, const int* gt_offsets_host,
                                       const float* cfg15_host, const float* grad_losses, const float* coef3,
                                       void* workspace, size_t workspace_bytes, float* da, float* dr, float* dscale,
                                       void* stream) {
    AtssGeom g;
    if (!layout8_host || !cfg15_host || !gt_offsets_host || !base_anchors_host) return BRCNN_EINVAL;
    const int st = fill_geom(g, batch, num_levels, heights, widths, strides, base_anchors_host, num_classes, gt_offsets_host,
                             layout8_host, cfg15_host);
    if (st) return st;
    return launch_loss_backward<AtssTraits>(g, a, r, scales, gt_inds, gts, gt_labels, grad_losses, coef3, workspace,
                                            workspace_bytes, da, dr, dscale, stream);
}
