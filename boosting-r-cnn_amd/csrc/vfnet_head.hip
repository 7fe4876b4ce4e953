// The VFNet head: VFNetHead (mmdet/models/dense_heads/vfnet_head.py) with VarifocalLoss (models/losses/varifocal_loss.py),
// trained on brcnn_atss_assign's gt_inds.
//
// One anchor per cell, regenerated where it is needed (row_head.h: anchor_of); only its centre is used: it is the
// reference's point (x * s, y * s) + s * center_offset.  The head leaves fp32 row tensors over all levels, level-major rows:
// R0 / R1 with 4 RAW distance logits in (l, t, r, b) order, A with the C class logits; D0 / D1 are dense (rows, 4) distances
// in pixels.
//
//   vfnet_star_offsets  : D0 = exp(scale_l * raw0) * reg_denom_l and the 18 offsets of the star-shaped deformable conv in the
//                         row layout of brcnn_deform_im2col_nhwc_g ([2t] = dy, [2t + 1] = dx of tap t), formed in
//                         star_dcn_offset's operation order; backward with dscale from block partials.
//   vfnet_refine        : D1 = exp(scale_refine_l * raw1) * D0 (D0 a constant) and its backward: the same two kernels.
//   vfnet_decode_levels : one thread per (image, pick, class) slot; D1 of the picked row, distance2bbox from the point, then
//                         decode_tail.h's store_candidate.  score = sigmoid(cls_c).
//   vfnet_loss_*        : VFNetHead.loss in the block-partial scheme of row_head.h: fixed order within a thread, LDS tree,
//                         one norm and one finalize workgroup; no float atomics, the same bits from run to run.  The dD
//                         kernel is this file's own.
//
// The geometry, the decode kernel, the loss forward and the dA kernels are row_head.h's, instantiated with VfTraits.
//
// The deformable kernels (deform.hip, deform_common.h) compare a sample coordinate with (-1, H) x (-1, W) in fp32 BEFORE any
// conversion to int, so a huge, infinite or NaN offset samples zero and indexes nothing: the offsets are not clamped here.
#include "box_iou.h"
#include "row_head.h"

namespace {

struct VfGeom : RowGeom {
    float base[BRCNN_MAX_LEVELS][4];
    float denom[BRCNN_MAX_LEVELS];
    float eps;
    int iou_weighted;
};

struct VfDecode : RowDecode {
    float base[BRCNN_MAX_LEVELS][4];
    const float* d0;                        // (rows, 4), device
};

// the device pointers the loss kernels read
struct VfRows {
    const float* __restrict__ a;
    const float* __restrict__ d0;
    const float* __restrict__ d1;
};

// -------------------------------------------------------------------------------------------- distances and star offsets
// STAR: d = exp(sc * raw) * denom_l, and the offsets; else d = exp(sc * raw) * d_in (the refinement)
template <bool STAR>
__global__ __launch_bounds__(256) void vfnet_dist_kernel(const VfGeom g, const float* __restrict__ raw, int sr, int off,
                                                        const float* __restrict__ scales, const float* __restrict__ d_in,
                                                        float f0, float f1, float* __restrict__ d_out,
                                                        float* __restrict__ offsets) {
    const long long rows = g.row0[g.L];
    for (long long row = (long long)blockIdx.x * blockDim.x + threadIdx.x; row < rows; row += (long long)gridDim.x * blockDim.x) {
        const int l = level_of_row(g, row);
        const float sc = scales[l];
        const float* x = raw + (size_t)row * sr + off;
        float d[4];
#pragma unroll
        for (int k = 0; k < 4; k++) d[k] = expf(x[k] * sc) * (STAR ? g.denom[l] : d_in[(size_t)row * 4 + k]);
        *reinterpret_cast<float4*>(d_out + (size_t)row * 4) = make_float4(d[0], d[1], d[2], d[3]);
        if (STAR) {
            // star_dcn_offset: (1 - gradient_mul) * d.detach() + gradient_mul * d, / stride, the signed entries, - base
            const float st = (float)g.stride[l];
            float q[4];
#pragma unroll
            for (int k = 0; k < 4; k++) q[k] = (f0 * d[k] + f1 * d[k]) / st;
            float* o = offsets + (size_t)row * 18;
#pragma unroll
            for (int t = 0; t < 9; t++) {
                const int ty = t / 3, tx = t % 3;
                const float vy = ty == 0 ? -1.0f * q[1] : (ty == 2 ? q[3] : 0.f);
                const float vx = tx == 0 ? -1.0f * q[0] : (tx == 2 ? q[2] : 0.f);
                o[2 * t] = vy - (float)(ty - 1);
                o[2 * t + 1] = vx - (float)(tx - 1);
            }
        }
    }
}

// one thread per row of d_raw (rows, sr): the 4 distance columns, zeros elsewhere; and per workgroup the partial of
// dscale_l = sum over the level's rows of d(scaled) * raw.  dd (rows, 4) and doff (rows, 18) may each be NULL (= zeros)
template <bool STAR>
__global__ __launch_bounds__(256) void vfnet_dist_backward_kernel(const VfGeom g, const float* __restrict__ raw, int sr,
                                                                 int off, const float* __restrict__ scales,
                                                                 const float* __restrict__ d, const float* __restrict__ dd,
                                                                 const float* __restrict__ doff, float f1,
                                                                 float* __restrict__ draw,
                                                                 float* __restrict__ dscale_partials) {
    __shared__ float red[CH_THREADS];
    const int blk = blockIdx.x, tid = threadIdx.x;
    int l = 0;
#pragma unroll
    for (int i = 1; i < BRCNN_MAX_LEVELS; i++)
        if (i < g.L && blk >= g.pblk0[i]) l = i;
    const long long rows = (long long)g.B * g.h[l] * g.w[l];
    const long long e0 = (long long)(blk - g.pblk0[l]) * CH_CHUNK;
    const float sc = scales[l], st = (float)g.stride[l];
    float acc = 0.f;
    for (int j = 0; j < CH_PER_THREAD; j++) {
        const long long e = e0 + (long long)j * CH_THREADS + tid;
        if (e >= rows) break;
        const size_t row = (size_t)(g.row0[l] + e);
        float gd[4] = {0.f, 0.f, 0.f, 0.f};
        if (dd) {
#pragma unroll
            for (int k = 0; k < 4; k++) gd[k] = dd[row * 4 + k];
        }
        if (STAR && doff) {
            const float* o = doff + row * 18;
            // the three entries per side, in channel order; the left and top sides enter with a minus sign
            const float gq[4] = {-((o[1] + o[7]) + o[13]), -((o[0] + o[2]) + o[4]), (o[5] + o[11]) + o[17],
                                 (o[12] + o[14]) + o[16]};
#pragma unroll
            for (int k = 0; k < 4; k++) gd[k] += f1 * (gq[k] / st);
        }
        const float* x = raw + row * sr + off;
        float* out = draw + row * sr;
        float dz[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            dz[k] = gd[k] * d[row * 4 + k];
            acc += dz[k] * x[k];
        }
        for (int ch = 0; ch < sr; ch++) {
            const int k = ch - off;
            out[ch] = (k >= 0 && k < 4) ? dz[k] * sc : 0.f;
        }
    }
    const float s = block_sum(acc, red, tid);
    if (tid == 0) dscale_partials[blk] = s;
}

// ------------------------------------------------------------------------------------------------------------------ loss
// what one row is: its image, its state and, for a positive, the point and the target box after the reference's round trip
// gt -> bbox2distance -> distance2bbox (not the identity in fp32)
struct VfCell {
    int b, gi;          // gi: index into the packed gts (positive), -1 otherwise (negative or invalid cell: background)
    float px, py;
    float4 gt;
};

__device__ __forceinline__ VfCell vf_locate(const VfGeom& g, const int* __restrict__ gt_inds, const float* __restrict__ gts,
                                            int l, long long r, bool want_targets) {
    VfCell o;
    const int hw = g.h[l] * g.w[l];
    o.b = (int)(r / hw);
    const int cell = (int)(r - (long long)o.b * hw);
    const int gi = gt_inds[(size_t)o.b * g.n + g.start[l] + cell];
    o.gi = (gi > 0 && gi <= g.gt_off[o.b + 1] - g.gt_off[o.b]) ? g.gt_off[o.b] + gi - 1 : -1;
    if (want_targets && o.gi >= 0) {
        const float4 an = anchor_of(g.base[l], g.w[l], g.stride[l], cell);
        o.px = (an.z + an.x) / 2.f;
        o.py = (an.w + an.y) / 2.f;
        const float4 gt = *reinterpret_cast<const float4*>(gts + (size_t)o.gi * 4);
        const float tl = o.px - gt.x, tt = o.py - gt.y, tr = gt.z - o.px, tb = gt.w - o.py;
        o.gt = make_float4(o.px - tl, o.py - tt, o.px + tr, o.py + tb);
    }
    return o;
}

__device__ __forceinline__ float4 vf_box(const VfCell& o, const float* __restrict__ d) {
    return make_float4(o.px - d[0], o.py - d[1], o.px + d[2], o.py + d[3]);
}

// aligned bbox_overlaps(box, target).clamp(min=1e-6): the weight of a positive's box loss and, from D1, its class target
__device__ __forceinline__ float vf_weight(const float4 p, const VfCell& o) {
    return fmaxf(pair_iou(p, (p.z - p.x) * (p.w - p.y), o.gt, (o.gt.z - o.gt.x) * (o.gt.w - o.gt.y)), 1e-6f);
}

// varifocal_loss of one (row, class) element.  At a positive's label (hit, q > 0): BCE(x, q) * q (iou_weighted) or BCE(x, q);
// elsewhere BCE(x, 0) * (alpha * sigmoid(x)^gamma).  With BWD the derivative w.r.t. x (q is a constant)
template <bool BWD>
__device__ __forceinline__ float vfl_elem(float x, bool hit, float q, float alpha, float gamma, bool iou_weighted) {
    const float p = sigmoidf_(x);
    if (hit) {
        if (!BWD) return iou_weighted ? bce_logits(x, q) * q : bce_logits(x, q);
        return iou_weighted ? (p - q) * q : p - q;
    }
    const float ce = softplusf_(x), mod = alpha * powf(p, gamma);
    if (!BWD) return ce * mod;
    return p * mod + ce * (gamma * mod * (1.f - p));
}

// Partial arrays of the loss forward: [VFL sum (class workgroups) | sum w_ini (1 - giou0) (point workgroups),
// sum w_rf (1 - giou1), sum w_ini, sum w_rf, n_pos]
struct VfTraits {
    using Geom = VfGeom;
    using Decode = VfDecode;
    using Rows = VfRows;
    using Cell = VfCell;
    static constexpr int PARTIALS = 5;
    static constexpr bool HAS_INVALID = false;      // an invalid cell counts as background
    static constexpr bool HAS_CENTERNESS = false;
    static constexpr bool HAS_QUALITY = true;

    static __device__ __forceinline__ int grad(const VfGeom&, int term, int) { return term; }        // g3 (3,)

    // distance2bbox from the point with D1 = exp(scale_refine * raw1) * D0 of the picked row
    static __device__ __forceinline__ float4 decode_box(const VfDecode& lv, int l, int cell, size_t row,
                                                        const float* __restrict__ raw, float sc) {
        const float4 an = anchor_of(lv.base[l], lv.width[l], lv.stride[l], cell);
        const float px = (an.z + an.x) / 2.f, py = (an.w + an.y) / 2.f;
        float d[4];
#pragma unroll
        for (int k = 0; k < 4; k++) d[k] = expf(raw[k] * sc) * lv.d0[row * 4 + k];
        return make_float4(px - d[0], py - d[1], px + d[2], py + d[3]);
    }

    static __device__ __forceinline__ VfCell locate(const VfGeom& g, const int* __restrict__ gt_inds,
                                                    const float* __restrict__ gts, int l, long long r, bool want_targets) {
        return vf_locate(g, gt_inds, gts, l, r, want_targets);
    }

    static __device__ __forceinline__ float quality(const VfGeom& g, const VfRows& in, const int* __restrict__ gt_inds,
                                                    const float* __restrict__ gts, int l, long long r, size_t row) {
        const VfCell o = vf_locate(g, gt_inds, gts, l, r, true);
        return vf_weight(vf_box(o, in.d1 + row * 4), o);
    }

    template <bool BWD>
    static __device__ __forceinline__ float cls_elem(const VfGeom& g, float x, bool hit, float q) {
        return vfl_elem<BWD>(x, hit, q, g.alpha, g.gamma, g.iou_weighted != 0);
    }

    static __device__ __forceinline__ void point_terms(const VfGeom& g, const VfRows& in, const VfCell& o, int, size_t row,
                                                       float* acc) {
        const float4 p0 = vf_box(o, in.d0 + row * 4), p1 = vf_box(o, in.d1 + row * 4);
        const float w0 = vf_weight(p0, o), w1 = vf_weight(p1, o);
        acc[0] += corner_box_loss<false>(true, g.eps, g.eps, p0.x, p0.y, p0.z, p0.w, o.gt.x, o.gt.y, o.gt.z, o.gt.w,
                                         nullptr) * w0;
        acc[1] += corner_box_loss<false>(true, g.eps, g.eps, p1.x, p1.y, p1.z, p1.w, o.gt.x, o.gt.y, o.gt.z, o.gt.w,
                                         nullptr) * w1;
        acc[2] += w0;
        acc[3] += w1;
        acc[4] += 1.f;
    }
};  // VfTraits

// norm3 = [number of positives of the batch, sum w_ini, sum w_rf], not clamped (the caller may average them over ranks);
// a count is an integer below 2^24, exact in fp32
__global__ __launch_bounds__(256) void vfnet_loss_norm_kernel(const VfGeom g, const float* __restrict__ partials,
                                                             float* __restrict__ norm3) {
    __shared__ float red[CH_THREADS];
    const int tid = threadIdx.x;
    const float n = term_sum(g, partials, 4, 1, red, tid), s0 = term_sum(g, partials, 2, 1, red, tid),
                s1 = term_sum(g, partials, 3, 1, red, tid);
    if (tid == 0) { norm3[0] = n; norm3[1] = s0; norm3[2] = s1; }
}

// losses (3) = [loss_cls, loss_bbox, loss_bbox_rf]; coef3 = [lw_cls / N, lw_bbox / S0, lw_rf / S1], each normaliser >= 1
__global__ __launch_bounds__(256) void vfnet_loss_finalize_kernel(const VfGeom g, const float* __restrict__ partials,
                                                                 const float* __restrict__ norm3, float* __restrict__ losses,
                                                                 float* __restrict__ coef3) {
    __shared__ float red[CH_THREADS];
    const int tid = threadIdx.x;
    const float N = fmaxf(norm3[0], 1.f), S0 = fmaxf(norm3[1], 1.f), S1 = fmaxf(norm3[2], 1.f);
    const float cls = term_sum(g, partials, 0, 0, red, tid), b0 = term_sum(g, partials, 0, 1, red, tid),
                b1 = term_sum(g, partials, 1, 1, red, tid);
    if (tid == 0) {
        losses[0] = g.lw_cls * (cls / N);
        losses[1] = g.lw_bbox * (b0 / S0);
        losses[2] = g.lw_ctr * (b1 / S1);
        coef3[0] = g.lw_cls / N;
        coef3[1] = g.lw_bbox / S0;
        coef3[2] = g.lw_ctr / S1;
    }
}

// one thread per row of dD0 and dD1 (rows, 4): the GIoU gradients of a positive through distance2bbox, zeros elsewhere
__global__ __launch_bounds__(256) void vfnet_loss_backward_d_kernel(const VfGeom g, const float* __restrict__ d0,
                                                                   const float* __restrict__ d1,
                                                                   const int* __restrict__ gt_inds,
                                                                   const float* __restrict__ gts, const float* __restrict__ gl,
                                                                   const float* __restrict__ coef3, float* __restrict__ dd0,
                                                                   float* __restrict__ dd1) {
    const long long rows = g.row0[g.L];
    for (long long row = (long long)blockIdx.x * blockDim.x + threadIdx.x; row < rows; row += (long long)gridDim.x * blockDim.x) {
        const int l = level_of_row(g, row);
        const VfCell o = vf_locate(g, gt_inds, gts, l, row - g.row0[l], true);
        float4 g0 = make_float4(0.f, 0.f, 0.f, 0.f), g1 = g0;
        if (o.gi >= 0) {
            const float4 p0 = vf_box(o, d0 + (size_t)row * 4), p1 = vf_box(o, d1 + (size_t)row * 4);
            const float k0 = gl[1] * coef3[1] * vf_weight(p0, o), k1 = gl[2] * coef3[2] * vf_weight(p1, o);
            float gp[4];
            // x1 = px - d[0], y1 = py - d[1], x2 = px + d[2], y2 = py + d[3]
            corner_box_loss<true>(true, g.eps, g.eps, p0.x, p0.y, p0.z, p0.w, o.gt.x, o.gt.y, o.gt.z, o.gt.w, gp);
            g0 = make_float4(k0 * -gp[0], k0 * -gp[1], k0 * gp[2], k0 * gp[3]);
            corner_box_loss<true>(true, g.eps, g.eps, p1.x, p1.y, p1.z, p1.w, o.gt.x, o.gt.y, o.gt.z, o.gt.w, gp);
            g1 = make_float4(k1 * -gp[0], k1 * -gp[1], k1 * gp[2], k1 * gp[3]);
        }
        *reinterpret_cast<float4*>(dd0 + (size_t)row * 4) = g0;
        *reinterpret_cast<float4*>(dd1 + (size_t)row * 4) = g1;
    }
}

// --------------------------------------------------------------------------------------------------------------- host
// cfg7_host: [VFL alpha, VFL gamma, iou_weighted, eps of the GIoU, loss_weight_cls, loss_weight_bbox, loss_weight_refine]
int fill_geom(VfGeom& g, int batch, int num_levels, const int* heights, const int* widths, const int* strides, const float* base,
              const float* denoms, int C, const int* gt_offsets_host, const float* cfg7) {
    const UnitStrides ones;
    const int st = fill_geom_common(g, batch, num_levels, heights, widths, strides ? strides : ones.v, C, gt_offsets_host, nullptr);
    if (st) return st;
    for (int l = 0; l < BRCNN_MAX_LEVELS; l++) {
        for (int k = 0; k < 4; k++) g.base[l][k] = (base && l < num_levels) ? base[4 * l + k] : 0.f;
        g.denom[l] = (denoms && l < num_levels) ? denoms[l] : 1.f;
        if (!(g.denom[l] > 0.f)) return BRCNN_EINVAL;
    }
    g.alpha = 0.75f; g.gamma = 2.f; g.iou_weighted = 1; g.eps = 1e-6f;
    if (cfg7) {
        g.alpha = cfg7[0]; g.gamma = cfg7[1]; g.iou_weighted = cfg7[2] != 0.f; g.eps = cfg7[3];
        g.lw_cls = cfg7[4]; g.lw_bbox = cfg7[5]; g.lw_ctr = cfg7[6];
        if (!(g.gamma >= 1.f) || !(g.eps > 0.f)) return BRCNN_EINVAL;
    }
    return 0;
}

template <bool STAR>
int launch_dist_backward(const VfGeom& g, const float* raw, int sr, int off, const float* scales, const float* d, const float* dd,
                         const float* doff, float f1, void* workspace, size_t workspace_bytes, float* draw, float* dscale,
                         void* stream) {
    if (!raw || !scales || !d || !workspace || !draw || !dscale || sr <= 0 || off < 0 || off + 4 > sr ||
        workspace_bytes < (size_t)g.pblk0[g.L] * sizeof(float))
        return BRCNN_EINVAL;
    float* dsp = (float*)workspace;
    hipLaunchKernelGGL(vfnet_dist_backward_kernel<STAR>, dim3(g.pblk0[g.L]), dim3(CH_THREADS), 0, (hipStream_t)stream, g, raw,
                       sr, off, scales, d, dd, doff, f1, draw, dsp);
    BRCNN_LAUNCH_CHECK();
    hipLaunchKernelGGL(rows_dscale_kernel<VfTraits>, dim3(1), dim3(CH_THREADS), 0, (hipStream_t)stream, g, dsp, dscale);
    BRCNN_LAUNCH_CHECK();
    return 0;
}

}  // namespace

BRCNN_API size_t brcnn_vfnet_rows_workspace_bytes(int batch, int num_levels, const int* heights, const int* widths) {
    VfGeom g;
    if (fill_geom(g, batch, num_levels, heights, widths, nullptr, nullptr, nullptr, 1, nullptr, nullptr)) return 0;
    return (size_t)g.pblk0[g.L] * sizeof(float);
}

BRCNN_API int brcnn_vfnet_star_offsets(const float* r0, int stride_r, int reg_off, const float* scales, int batch,
                                       int num_levels, const int* heights, const int* widths, const int* strides,
                                       const float* denoms_host, float f0, float f1, float* d0, float* offsets, void* stream) {
    VfGeom g;
    if (!strides || !denoms_host) return BRCNN_EINVAL;
    const int st = fill_geom(g, batch, num_levels, heights, widths, strides, nullptr, denoms_host, 1, nullptr, nullptr);
    if (st) return st;
    if (!r0 || !scales || !d0 || !offsets || stride_r <= 0 || reg_off < 0 || reg_off + 4 > stride_r) return BRCNN_EINVAL;
    hipLaunchKernelGGL(vfnet_dist_kernel<true>, dim3(rows_grid(g.row0[g.L])), dim3(256), 0, (hipStream_t)stream, g, r0, stride_r,
                       reg_off, scales, (const float*)nullptr, f0, f1, d0, offsets);
    BRCNN_LAUNCH_CHECK();
    return 0;
}

BRCNN_API int brcnn_vfnet_star_offsets_backward(const float* r0, int stride_r, int reg_off, const float* scales, int batch,
                                                int num_levels, const int* heights, const int* widths, const int* strides,
                                                float f1, const float* d0, const float* dd0, const float* doffsets,
                                                void* workspace, size_t workspace_bytes, float* dr0, float* dscale,
                                                void* stream) {
    VfGeom g;
    if (!strides) return BRCNN_EINVAL;
    const int st = fill_geom(g, batch, num_levels, heights, widths, strides, nullptr, nullptr, 1, nullptr, nullptr);
    if (st) return st;
    return launch_dist_backward<true>(g, r0, stride_r, reg_off, scales, d0, dd0, doffsets, f1, workspace, workspace_bytes, dr0,
                                      dscale, stream);
}

BRCNN_API int brcnn_vfnet_refine(const float* r1, int stride_r, int reg_off, const float* scales_refine, int batch,
                                 int num_levels, const int* heights, const int* widths, const float* d0, float* d1,
                                 void* stream) {
    VfGeom g;
    const int st = fill_geom(g, batch, num_levels, heights, widths, nullptr, nullptr, nullptr, 1, nullptr, nullptr);
    if (st) return st;
    if (!r1 || !scales_refine || !d0 || !d1 || stride_r <= 0 || reg_off < 0 || reg_off + 4 > stride_r) return BRCNN_EINVAL;
    hipLaunchKernelGGL(vfnet_dist_kernel<false>, dim3(rows_grid(g.row0[g.L])), dim3(256), 0, (hipStream_t)stream, g, r1, stride_r,
                       reg_off, scales_refine, d0, 0.f, 0.f, d1, (float*)nullptr);
    BRCNN_LAUNCH_CHECK();
    return 0;
}

BRCNN_API int brcnn_vfnet_refine_backward(const float* r1, int stride_r, int reg_off, const float* scales_refine, int batch,
                                          int num_levels, const int* heights, const int* widths, const float* d1,
                                          const float* dd1, void* workspace, size_t workspace_bytes, float* dr1, float* dscale,
                                          void* stream) {
    VfGeom g;
    const int st = fill_geom(g, batch, num_levels, heights, widths, nullptr, nullptr, nullptr, 1, nullptr, nullptr);
    if (st) return st;
    return launch_dist_backward<false>(g, r1, stride_r, reg_off, scales_refine, d1, dd1, nullptr, 0.f, workspace, workspace_bytes,
                                       dr1, dscale, stream);
}

BRCNN_API int brcnn_vfnet_decode_levels(const int64_t* const* topk_inds, const int* counts, const float* a, const float* r1,
                                        const int* layout4_host, const float* scales_refine, int batch, int num_levels,
                                        const int* heights, const int* widths, const int* strides,
                                        const float* base_anchors_host, const float* d0, int num_classes,
                                        const float* max_shape, const float* scale_factor, float score_thr, float* boxes,
                                        float* scores, int64_t* labels, uint8_t* valid, int32_t* n_valid, void* stream) {
    if (!a || !r1 || !d0 || !scales_refine || !base_anchors_host || !max_shape || !boxes || !scores || !labels || !valid ||
        !n_valid || num_classes <= 0 || !layout4_ok(layout4_host, num_classes, 4))
        return BRCNN_EINVAL;
    VfDecode lv = {};
    const int st = fill_decode_picks(lv, topk_inds, counts, batch, num_levels, heights, widths, strides, num_classes, score_thr);
    if (st) return st;
    lv.lay = make_layout4(layout4_host);
    lv.d0 = d0;
    fill_decode_base(lv, base_anchors_host, num_levels);
    return launch_decode_levels<VfTraits>(lv, batch, a, r1, scales_refine, max_shape, scale_factor, boxes, scores, labels, valid,
                                          n_valid, stream);
}

BRCNN_API size_t brcnn_vfnet_loss_workspace_bytes(int batch, int num_levels, const int* heights, const int* widths,
                                                  int num_classes) {
    VfGeom g;
    if (fill_geom(g, batch, num_levels, heights, widths, nullptr, nullptr, nullptr, num_classes, nullptr, nullptr)) return 0;
    return loss_workspace_bytes<VfTraits>(g);
}

BRCNN_API int brcnn_vfnet_loss_forward(const float* a, int stride_a, int cls_off, const float* d0, const float* d1, int batch,
                                       int num_levels, const int* heights, const int* widths, const int* strides,
                                       const float* base_anchors_host, int num_classes, const int32_t* gt_inds,
                                       const float* gts, const int64_t* gt_labels, const int* gt_offsets_host,
                                       const float* cfg7_host, void* workspace, size_t workspace_bytes, float* norm3,
                                       void* stream) {
    VfGeom g;
    if (!cfg7_host || !gt_offsets_host || !base_anchors_host || !strides) return BRCNN_EINVAL;
    const int st = fill_geom(g, batch, num_levels, heights, widths, strides, base_anchors_host, nullptr, num_classes,
                             gt_offsets_host, cfg7_host);
    if (st) return st;
    if (!a || !d0 || !d1 || !gt_inds || !workspace || !norm3 || ((!gts || !gt_labels) && g.gt_off[batch] > 0) ||
        stride_a <= 0 || cls_off < 0 || cls_off + num_classes > stride_a || workspace_bytes < loss_workspace_bytes<VfTraits>(g))
        return BRCNN_EINVAL;
    g.lay.sa = stride_a; g.lay.cls_off = cls_off;
    float* partials = (float*)workspace;
    const int fs = launch_loss_forward<VfTraits>(g, VfRows{a, d0, d1}, gt_inds, gts, gt_labels, partials, stream);
    if (fs) return fs;
    hipLaunchKernelGGL(vfnet_loss_norm_kernel, dim3(1), dim3(CH_THREADS), 0, (hipStream_t)stream, g, partials, norm3);
    BRCNN_LAUNCH_CHECK();
    return 0;
}

BRCNN_API int brcnn_vfnet_loss_finalize(const void* workspace, size_t workspace_bytes, const float* norm3, int batch,
                                        int num_levels, const int* heights, const int* widths, int num_classes,
                                        const float* cfg7_host, float* losses, float* coef3, void* stream) {
    VfGeom g;
    if (!cfg7_host) return BRCNN_EINVAL;
    const int st = fill_geom(g, batch, num_levels, heights, widths, nullptr, nullptr, nullptr, num_classes, nullptr, cfg7_host);
    if (st) return st;
    if (!workspace || !norm3 || !losses || !coef3 || workspace_bytes < loss_workspace_bytes<VfTraits>(g)) return BRCNN_EINVAL;
    hipLaunchKernelGGL(vfnet_loss_finalize_kernel, dim3(1), dim3(CH_THREADS), 0, (hipStream_t)stream, g, (const float*)workspace,
                       norm3, losses, coef3);
    BRCNN_LAUNCH_CHECK();
    return 0;
}

BRCNN_API int brcnn_vfnet_loss_backward(const float* a, int stride_a, int cls_off, const float* d0, const float* d1, int batch,
                                        int num_levels, const int* heights, const int* widths, const int* strides,
                                        const float* base_anchors_host, int num_classes, const int32_t* gt_inds,
                                        const float* gts, const int64_t* gt_labels, const int* gt_offsets_host,
                                        const float* cfg7_host, const float* grad_losses, const float* coef3, float* da,
                                        float* dd0, float* dd1, void* stream) {
    VfGeom g;
    if (!cfg7_host || !gt_offsets_host || !base_anchors_host || !strides) return BRCNN_EINVAL;
    const int st = fill_geom(g, batch, num_levels, heights, widths, strides, base_anchors_host, nullptr, num_classes,
                             gt_offsets_host, cfg7_host);
    if (st) return st;
    if (!a || !d0 || !d1 || !gt_inds || !grad_losses || !coef3 || !da || !dd0 || !dd1 ||
        ((!gts || !gt_labels) && g.gt_off[batch] > 0) || stride_a <= 0 || cls_off < 0 || cls_off + num_classes > stride_a)
        return BRCNN_EINVAL;
    g.lay.sa = stride_a; g.lay.cls_off = cls_off;
    const int as = launch_loss_backward_a<VfTraits>(g, VfRows{a, d0, d1}, gt_inds, gts, gt_labels, grad_losses, coef3, da, stream);
    if (as) return as;
    hipLaunchKernelGGL(vfnet_loss_backward_d_kernel, dim3(rows_grid(g.row0[g.L])), dim3(256), 0, (hipStream_t)stream, g, d0, d1,
                       gt_inds, gts, grad_losses, coef3, dd0, dd1);
    BRCNN_LAUNCH_CHECK();
    return 0;
}
