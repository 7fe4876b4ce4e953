// The sampled RPN loss of the Faster R-CNN baseline (RPNHead over AnchorHead.loss,
// mmdet/models/dense_heads/anchor_head.py:373-497 with a RandomSampler of 256 anchors per image,
// core/bbox/samplers/{base_sampler.py:35-102, random_sampler.py:32-82}):
//
//   rpn_sampled_draw     : per image the positive (gt_inds > 0) and negative (gt_inds == 0) candidates
//                          compacted in index order (torch.nonzero order), then the host-drawn picks
//                          gathered into `drawn` (batch, num): positives first, then negatives, -1 after.
//                          The host knows the candidate counts (brcnn_assign_max_iou's counts) and draws
//                          `perm` with the reference's randperm calls, exactly as for brcnn_rcnn_sample.
//   rpn_sampled_forward  : one thread per drawn slot: w * bce_with_logits(x, is_pos) and, for a positive,
//                          sum_4 l1 | smooth_l1(pred - bbox2delta(anchor, gt)); anchors regenerated from
//                          base anchor + cell * stride.  Terms go to a (batch*num, 2) table.
//   rpn_sampled_finalize : one workgroup sums the table in a fixed order (strided per-thread sums, LDS
//                          tree) and scales by loss_weight / num_total_samples.  No float atomics: the
//                          result is bit-identical from run to run.
//   rpn_sampled_backward : dy zeroed, then one thread per drawn slot writes its five gradients (a drawn
//                          anchor occurs once, so no two threads meet).
//
// y is the fused head output of all levels, level-major rows (level l: batch * h_l * w_l rows), columns
// [objectness A | deltas 4A | padding]; the flat anchor index of an image is the reference's
// (level, cell row-major, anchor) order.
#include "common.h"
#include <math.h>

namespace {

struct SampledGeom {
    int L, A, B, n, num, ystride;
    int h[BRCNN_MAX_LEVELS], w[BRCNN_MAX_LEVELS], sw[BRCNN_MAX_LEVELS], sh[BRCNN_MAX_LEVELS];
    int start[BRCNN_MAX_LEVELS + 1];        // first anchor of each level within an image
    long long row0[BRCNN_MAX_LEVELS];       // first row of each level in y
    const float* base[BRCNN_MAX_LEVELS];
    int gt_off[BRCNN_MAX_IMAGES + 1];
    float pos_weight, beta, mean[4], std[4];
};

__global__ __launch_bounds__(1024) void rpn_sampled_draw_kernel(const int* __restrict__ gt_inds, int n, int num,
                                                               int num_pos, float neg_pos_ub,
                                                               const int* __restrict__ perm, int* __restrict__ lists,
                                                               int* __restrict__ drawn) {
    __shared__ int wsum_p[16], wsum_n[16];
    __shared__ int s_base[2];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int* list_p = lists + (size_t)b * 2 * n;
    int* list_n = list_p + n;
    const int* gi_row = gt_inds + (size_t)b * n;
    if (tid < 2) s_base[tid] = 0;
    __syncthreads();
    for (int t0 = 0; t0 < n; t0 += 1024) {
        const int t = t0 + tid;
        const int gi = t < n ? gi_row[t] : -1;
        const int vp = gi > 0 ? 1 : 0, vn = gi == 0 ? 1 : 0;
        int ip = vp, in = vn;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int op = __shfl_up(ip, d, 64), on = __shfl_up(in, d, 64);
            if (lane >= d) { ip += op; in += on; }
        }
        if (lane == 63) { wsum_p[wave] = ip; wsum_n[wave] = in; }
        __syncthreads();
        int offp = 0, offn = 0, totp = 0, totn = 0;
        for (int w = 0; w < 16; w++) {
            if (w < wave) { offp += wsum_p[w]; offn += wsum_n[w]; }
            totp += wsum_p[w];
            totn += wsum_n[w];
        }
        if (vp) list_p[s_base[0] + offp + ip - 1] = t;
        if (vn) list_n[s_base[1] + offn + in - 1] = t;
        __syncthreads();
        if (tid == 0) { s_base[0] += totp; s_base[1] += totn; }
        __syncthreads();
    }
    const int npos = s_base[0], nneg = s_base[1];
    const int spos = min(npos, num_pos);
    int eneg = num - spos;
    if (neg_pos_ub >= 0.f) eneg = min(eneg, (int)(neg_pos_ub * (float)max(1, spos)));
    const int sneg = min(nneg, eneg);
    const int* perm_p = perm + (size_t)b * (num_pos + num);
    const int* perm_n = perm_p + num_pos;
    __threadfence_block();
    __syncthreads();
    int* out = drawn + (size_t)b * num;
    for (int j = tid; j < num; j += 1024) {
        int v = -1;
        if (j < spos) {
            v = list_p[npos > num_pos ? min(max(perm_p[j], 0), npos - 1) : j];
        } else if (j < spos + sneg) {
            const int q = j - spos;
            v = list_n[nneg > eneg ? min(max(perm_n[q], 0), nneg - 1) : q];
        }
        out[j] = v;
    }
}

// what one drawn slot needs: where its anchor sits in y, whether it is positive, and the encoded target
struct Slot {
    bool live, pos;
    long long row;
    int a;
    float t[4];
};

__device__ __forceinline__ Slot load_slot(const SampledGeom& g, const int* __restrict__ drawn,
                                          const int* __restrict__ gt_inds, const float* __restrict__ gts, int s) {
    Slot o;
    o.live = false; o.pos = false; o.row = 0; o.a = 0;
    o.t[0] = o.t[1] = o.t[2] = o.t[3] = 0.f;
    const int b = s / g.num;
    const int idx = drawn[s];
    if (idx < 0 || idx >= g.n) return o;
    const int gi = gt_inds[(size_t)b * g.n + idx];
    if (gi < 0) return o;
    int l = 0;
#pragma unroll
    for (int i = 1; i < BRCNN_MAX_LEVELS; i++)
        if (i < g.L && idx >= g.start[i]) l = i;
    const int local = idx - g.start[l];
    const int a = local % g.A, cell = local / g.A;
    o.live = true;
    o.a = a;
    o.row = g.row0[l] + (long long)b * g.h[l] * g.w[l] + cell;
    const int G = g.gt_off[b + 1] - g.gt_off[b];
    if (gi > 0 && gi <= G && gts) {
        o.pos = true;
        const int cx = cell % g.w[l], cy = cell / g.w[l];
        const float sx = (float)(cx * g.sw[l]), sy = (float)(cy * g.sh[l]);
        const float4 ba = *reinterpret_cast<const float4*>(g.base[l] + a * 4);
        const float x1 = ba.x + sx, y1 = ba.y + sy, x2 = ba.z + sx, y2 = ba.w + sy;
        const float4 gt = *reinterpret_cast<const float4*>(gts + (size_t)(g.gt_off[b] + gi - 1) * 4);
        // bbox2delta (delta_xywh_bbox_coder.py:99-141)
        const float px = (x1 + x2) * 0.5f, py = (y1 + y2) * 0.5f;
        const float pw = x2 - x1, ph = y2 - y1;
        const float gx = (gt.x + gt.z) * 0.5f, gy = (gt.y + gt.w) * 0.5f;
        const float gw = gt.z - gt.x, gh = gt.w - gt.y;
        o.t[0] = ((gx - px) / pw - g.mean[0]) / g.std[0];
        o.t[1] = ((gy - py) / ph - g.mean[1]) / g.std[1];
        o.t[2] = (logf(gw / pw) - g.mean[2]) / g.std[2];
        o.t[3] = (logf(gh / ph) - g.mean[3]) / g.std[3];
    }
    return o;
}

__global__ __launch_bounds__(256) void rpn_sampled_forward_kernel(const SampledGeom g, const float* __restrict__ y,
                                                                 const int* __restrict__ drawn,
                                                                 const int* __restrict__ gt_inds,
                                                                 const float* __restrict__ gts,
                                                                 float* __restrict__ terms) {
    const int total = g.B * g.num;
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= total) return;
    const Slot o = load_slot(g, drawn, gt_inds, gts, s);
    float lc = 0.f, lb = 0.f;
    if (o.live) {
        const float* yr = y + (size_t)o.row * g.ystride;
        const float x = yr[o.a];
        const float w = (o.pos && g.pos_weight > 0.f) ? g.pos_weight : 1.f;
        // binary_cross_entropy_with_logits: max(x, 0) - x * t + log1p(exp(-|x|))
        lc = w * (fmaxf(x, 0.f) - (o.pos ? x : 0.f) + log1pf(expf(-fabsf(x))));
        if (o.pos) {
            const float* pr = yr + g.A + 4 * o.a;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const float d = fabsf(pr[k] - o.t[k]);
                lb += (g.beta > 0.f && d < g.beta) ? 0.5f * d * d / g.beta : d - 0.5f * g.beta;
            }
        }
    }
    terms[2 * (size_t)s] = lc;
    terms[2 * (size_t)s + 1] = lb;
}

// losses2 = [lw_cls, lw_bbox] / avg_factor * column sums of terms; coef2 = the two scale factors
__global__ __launch_bounds__(256) void rpn_sampled_finalize_kernel(const float* __restrict__ terms, int total,
                                                                  float k_cls, float k_bbox,
                                                                  float* __restrict__ losses2,
                                                                  float* __restrict__ coef2) {
    __shared__ float sc[256], sb[256];
    const int tid = threadIdx.x;
    float c = 0.f, b = 0.f;
    for (int s = tid; s < total; s += 256) {
        c += terms[2 * (size_t)s];
        b += terms[2 * (size_t)s + 1];
    }
    sc[tid] = c;
    sb[tid] = b;
    __syncthreads();
    for (int d = 128; d > 0; d >>= 1) {
        if (tid < d) { sc[tid] += sc[tid + d]; sb[tid] += sb[tid + d]; }
        __syncthreads();
    }
    if (tid == 0) {
        losses2[0] = sc[0] * k_cls;
        losses2[1] = sb[0] * k_bbox;
        coef2[0] = k_cls;
        coef2[1] = k_bbox;
    }
}

__global__ __launch_bounds__(256) void rpn_sampled_backward_kernel(const SampledGeom g, const float* __restrict__ y,
                                                                  const int* __restrict__ drawn,
                                                                  const int* __restrict__ gt_inds,
                                                                  const float* __restrict__ gts,
                                                                  const float* __restrict__ g2,
                                                                  const float* __restrict__ coef2,
                                                                  float* __restrict__ dy) {
    const int total = g.B * g.num;
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= total) return;
    const Slot o = load_slot(g, drawn, gt_inds, gts, s);
    if (!o.live) return;
    const float kc = g2[0] * coef2[0], kb = g2[1] * coef2[1];
    const float* yr = y + (size_t)o.row * g.ystride;
    float* dr = dy + (size_t)o.row * g.ystride;
    const float x = yr[o.a];
    const float w = (o.pos && g.pos_weight > 0.f) ? g.pos_weight : 1.f;
    const float sig = x >= 0.f ? 1.f / (1.f + expf(-x)) : expf(x) / (1.f + expf(x));
    dr[o.a] = kc * w * (sig - (o.pos ? 1.f : 0.f));
    if (o.pos) {
        const float* pr = yr + g.A + 4 * o.a;
        float* dp = dr + g.A + 4 * o.a;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const float diff = pr[k] - o.t[k];
            const float d = fabsf(diff);
            float gk;
            if (g.beta > 0.f && d < g.beta) gk = diff / g.beta;
            else gk = diff > 0.f ? 1.f : (diff < 0.f ? -1.f : 0.f);
            dp[k] = kb * gk;
        }
    }
}

// cfg13_host: [pos_weight, smooth_l1_beta (0: L1), means x4, stds x4, loss_weight_cls, loss_weight_bbox,
// num_total_samples]
int fill_geom(SampledGeom& g, int ystride, int batch, int num_levels, const int* heights, const int* widths,
              const int* strides_w, const int* strides_h, const float* const* base_anchors, int A, int num,
              const int* gt_offsets_host, const float* cfg, long long* rows_out) {
    if (batch <= 0 || batch > BRCNN_MAX_IMAGES || num_levels <= 0 || num_levels > BRCNN_MAX_LEVELS || A <= 0 ||
        num <= 0 || !heights || !widths || !strides_w || !strides_h || !base_anchors || !gt_offsets_host || !cfg ||
        ystride < 5 * A)
        return BRCNN_EINVAL;
    g.L = num_levels; g.A = A; g.B = batch; g.num = num; g.ystride = ystride;
    long long anchors = 0, rows = 0;
    for (int l = 0; l < num_levels; l++) {
        if (heights[l] <= 0 || widths[l] <= 0 || !base_anchors[l]) return BRCNN_EINVAL;
        g.h[l] = heights[l]; g.w[l] = widths[l]; g.sw[l] = strides_w[l]; g.sh[l] = strides_h[l];
        g.base[l] = base_anchors[l];
        g.start[l] = (int)anchors;
        g.row0[l] = rows;
        anchors += (long long)heights[l] * widths[l] * A;
        rows += (long long)batch * heights[l] * widths[l];
        if (anchors > 0x7fffffffLL) return BRCNN_EINVAL;
    }
    for (int l = num_levels; l < BRCNN_MAX_LEVELS; l++) {
        g.h[l] = g.w[l] = 1; g.sw[l] = g.sh[l] = 0; g.base[l] = nullptr; g.row0[l] = 0;
    }
    for (int l = num_levels; l <= BRCNN_MAX_LEVELS; l++) g.start[l] = (int)anchors;
    g.n = (int)anchors;
    for (int b = 0; b <= batch; b++) {
        if (gt_offsets_host[b] < 0 || (b > 0 && gt_offsets_host[b] < gt_offsets_host[b - 1])) return BRCNN_EINVAL;
        g.gt_off[b] = gt_offsets_host[b];
    }
    for (int b = batch + 1; b <= BRCNN_MAX_IMAGES; b++) g.gt_off[b] = gt_offsets_host[batch];
    g.pos_weight = cfg[0]; g.beta = cfg[1];
    for (int i = 0; i < 4; i++) {
        g.mean[i] = cfg[2 + i]; g.std[i] = cfg[6 + i];
        if (!(g.std[i] > 0.f)) return BRCNN_EINVAL;
    }
    if (!(cfg[12] > 0.f) || g.beta < 0.f) return BRCNN_EINVAL;
    if (rows_out) *rows_out = rows;
    return 0;
}

}  // namespace

BRCNN_API size_t brcnn_rpn_sampled_workspace_bytes(int batch, int anchors_per_image, int num) {
    if (batch <= 0 || anchors_per_image <= 0 || num <= 0) return 0;
    // candidate lists (batch, 2, n) int32 + loss terms (batch * num, 2) fp32
    return (size_t)batch * 2 * anchors_per_image * sizeof(int32_t) + (size_t)batch * num * 2 * sizeof(float);
}

BRCNN_API int brcnn_rpn_sampled_draw(const int32_t* gt_inds, int anchors_per_image, int batch, int num,
                                     int num_expected_pos, float neg_pos_ub, const int32_t* perm, void* workspace,
                                     size_t workspace_bytes, int32_t* drawn, void* stream) {
    if (!gt_inds || !perm || !workspace || !drawn || batch <= 0 || batch > BRCNN_MAX_IMAGES || anchors_per_image <= 0 ||
        num <= 0 || num_expected_pos < 0 || num_expected_pos > num ||
        workspace_bytes < brcnn_rpn_sampled_workspace_bytes(batch, anchors_per_image, num))
        return BRCNN_EINVAL;
    hipLaunchKernelGGL(rpn_sampled_draw_kernel, dim3(batch), dim3(1024), 0, (hipStream_t)stream, gt_inds,
                       anchors_per_image, num, num_expected_pos, neg_pos_ub, perm, (int*)workspace, drawn);
    BRCNN_LAUNCH_CHECK();
    return 0;
}

BRCNN_API int brcnn_rpn_sampled_loss_forward(const float* y, int ystride, int batch, int num_levels, const int* heights,
                                             const int* widths, const int* strides_w, const int* strides_h,
                                             const float* const* base_anchors, int anchors_per_cell,
                                             const int32_t* gt_inds, const float* gts, const int* gt_offsets_host,
                                             const int32_t* drawn, int num, const float* cfg13_host, void* workspace,
                                             size_t workspace_bytes, void* stream) {
    SampledGeom g;
    const int st = fill_geom(g, ystride, batch, num_levels, heights, widths, strides_w, strides_h, base_anchors,
                             anchors_per_cell, num, gt_offsets_host, cfg13_host, nullptr);
    if (st) return st;
    if (!y || !gt_inds || !drawn || !workspace || (!gts && g.gt_off[batch] > 0) ||
        workspace_bytes < brcnn_rpn_sampled_workspace_bytes(batch, g.n, num))
        return BRCNN_EINVAL;
    float* terms = (float*)((char*)workspace + (size_t)batch * 2 * g.n * sizeof(int32_t));
    const int total = batch * num;
    hipLaunchKernelGGL(rpn_sampled_forward_kernel, dim3((total + 255) / 256), dim3(256), 0, (hipStream_t)stream, g, y,
                       drawn, gt_inds, gts, terms);
    BRCNN_LAUNCH_CHECK();
    return 0;
}

BRCNN_API int brcnn_rpn_sampled_loss_finalize(const void* workspace, int batch, int anchors_per_image, int num,
                                              const float* cfg13_host, float* losses2, float* coef2, void* stream) {
    if (!workspace || !cfg13_host || !losses2 || !coef2 || batch <= 0 || anchors_per_image <= 0 || num <= 0 ||
        !(cfg13_host[12] > 0.f))
        return BRCNN_EINVAL;
    const float* terms = (const float*)((const char*)workspace + (size_t)batch * 2 * anchors_per_image * sizeof(int32_t));
    hipLaunchKernelGGL(rpn_sampled_finalize_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, terms, batch * num,
                       cfg13_host[10] / cfg13_host[12], cfg13_host[11] / cfg13_host[12], losses2, coef2);
    BRCNN_LAUNCH_CHECK();
    return 0;
}

BRCNN_API int brcnn_rpn_sampled_loss_backward(const float* y, int ystride, int batch, int num_levels, const int* heights,
                                              const int* widths, const int* strides_w, const int* strides_h,
                                              const float* const* base_anchors, int anchors_per_cell,
                                              const int32_t* gt_inds, const float* gts, const int* gt_offsets_host,
                                              const int32_t* drawn, int num, const float* cfg13_host, const float* g2,
                                              const float* coef2, float* dy, void* stream) {
    SampledGeom g;
    long long rows = 0;
    const int st = fill_geom(g, ystride, batch, num_levels, heights, widths, strides_w, strides_h, base_anchors,
                             anchors_per_cell, num, gt_offsets_host, cfg13_host, &rows);
    if (st) return st;
    if (!y || !gt_inds || !drawn || !g2 || !coef2 || !dy || (!gts && g.gt_off[batch] > 0)) return BRCNN_EINVAL;
    BRCNN_HIP_CHECK(hipMemsetAsync(dy, 0, (size_t)rows * ystride * sizeof(float), (hipStream_t)stream));
    const int total = batch * num;
    hipLaunchKernelGGL(rpn_sampled_backward_kernel, dim3((total + 255) / 256), dim3(256), 0, (hipStream_t)stream, g, y,
                       drawn, gt_inds, gts, g2, coef2, dy);
    BRCNN_LAUNCH_CHECK();
    return 0;
}
