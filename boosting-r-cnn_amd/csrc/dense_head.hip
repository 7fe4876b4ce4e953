// The dense (single-stage) detection head: RetinaHead over AnchorHead
// (mmdet/models/dense_heads/anchor_head.py; retina_head.py adds only the two conv towers).
//
//   dense_score         : score[r * A + a] = max_c sigmoid(cls[r, a * C + c])            (anchor_head.py:646-669:
//                         `scores = cls_score.sigmoid(); max_scores, _ = scores.max(-1)`).  The maximum is taken over
//                         the fp32 SIGMOID VALUES, so two logits that round to one sigmoid tie, and the top-k's
//                         index-ascending rule decides, as `topk` on those values does.
//   dense_decode_levels : everything between the top-k and multiclass_nms (anchor_head.py:672-710,
//                         core/post_processing/bbox_nms.py:34-62) for all levels and images in one launch: the picked
//                         anchor regenerated from base anchor + cell * stride, delta2bbox
//                         (delta_xywh_bbox_coder.py:145-272, the reference's operation order), clip to the image,
//                         `/ scale_factor`, and the fan-out to classes in (level, pick, class) order -- the order of
//                         `valid_mask.nonzero()` -- with score = the class sigmoid, valid = score > score_thr.
//   dense_loss_*        : AnchorHead.loss without a sampler (anchor_head.py:373-491 with PseudoSampler): sigmoid focal
//                         loss over every weighted (anchor, class) pair, L1 / SmoothL1 on pred - bbox2delta(anchor, gt)
//                         over the positives, both divided by num_total_pos = sum over images of max(n_pos, 1)
//                         (anchor_head.py:354, :469), which is counted and inverted on the device.
//
// Work is laid out along the NHWC rows: consecutive lanes read consecutive channels.  The loss sums go block partial
// (fixed order within a thread, LDS tree) -> one finalize workgroup (strided sums, LDS tree): no float atomics, the
// same bits from run to run.
#include "decode_tail.h"
#include <float.h>
#include <math.h>

namespace {

constexpr int DL_THREADS = 256;
constexpr int DL_PER_THREAD = 8;
constexpr int DL_CHUNK = DL_THREADS * DL_PER_THREAD;        // elements one workgroup sums
constexpr int DL_SEGS = 2 * BRCNN_MAX_LEVELS;               // (level, term) pairs: 2 * l = class term, 2 * l + 1 = box term

__global__ __launch_bounds__(256) void dense_score_kernel(const float* __restrict__ cls, float* __restrict__ score,
                                                         long long rows, int A, int C, int cls_stride) {
    const long long n = rows * A;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const long long r = i / A;
        const int a = (int)(i - r * A);
        const float* x = cls + r * cls_stride + a * C;
        float m = 1.f / (1.f + expf(-x[0]));
        for (int c = 1; c < C; c++) m = fmaxf(m, 1.f / (1.f + expf(-x[c])));
        score[i] = m;
    }
}

struct DenseDecode {
    int num, A, C, T;
    const int64_t* inds[BRCNN_MAX_LEVELS];
    const float* cls[BRCNN_MAX_LEVELS];
    const float* reg[BRCNN_MAX_LEVELS];
    const float* base[BRCNN_MAX_LEVELS];
    int cls_stride[BRCNN_MAX_LEVELS], reg_stride[BRCNN_MAX_LEVELS], hw[BRCNN_MAX_LEVELS], width[BRCNN_MAX_LEVELS];
    int stride_w[BRCNN_MAX_LEVELS], stride_h[BRCNN_MAX_LEVELS], col0[BRCNN_MAX_LEVELS + 1];
    float mean[4], std[4], max_ratio, score_thr;
};

__global__ __launch_bounds__(256) void dense_decode_levels_kernel(const DenseDecode lv, int batch,
                                                                 const float* __restrict__ max_shape,
                                                                 const float* __restrict__ scale,
                                                                 float* __restrict__ boxes, float* __restrict__ scores,
                                                                 int64_t* __restrict__ labels, uint8_t* __restrict__ valid,
                                                                 int* __restrict__ n_valid) {
    const long long per_image = (long long)lv.T * lv.C;
    const long long total = (long long)batch * per_image;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x) {
        const int b = (int)(t / per_image);
        const long long q = t - (long long)b * per_image;
        const int col = (int)(q / lv.C), c = (int)(q - (long long)col * lv.C);
        int l = 0;
#pragma unroll
        for (int i = 1; i < BRCNN_MAX_LEVELS; i++)
            if (i < lv.num && col >= lv.col0[i]) l = i;
        const int count = lv.col0[l + 1] - lv.col0[l];
        long long idx = lv.inds[l][(size_t)b * count + (col - lv.col0[l])];
        const long long hwA = (long long)lv.hw[l] * lv.A;
        idx = idx < 0 ? 0 : (idx >= hwA ? hwA - 1 : idx);       // (a picked index is an anchor of the level)
        const int a = (int)(idx % lv.A);
        const long long cell = idx / lv.A;
        const size_t row = (size_t)b * lv.hw[l] + cell;
        const float s = 1.f / (1.f + expf(-lv.cls[l][row * lv.cls_stride[l] + a * lv.C + c]));
        const int cx = (int)(cell % lv.width[l]), cy = (int)(cell / lv.width[l]);
        const float sx = (float)(cx * lv.stride_w[l]), sy = (float)(cy * lv.stride_h[l]);
        const float4 ba = *reinterpret_cast<const float4*>(lv.base[l] + a * 4);
        const float x1 = ba.x + sx, y1 = ba.y + sy, x2 = ba.z + sx, y2 = ba.w + sy;
        const float* d = lv.reg[l] + row * lv.reg_stride[l] + a * 4;
        const float dx = d[0] * lv.std[0] + lv.mean[0];
        const float dy = d[1] * lv.std[1] + lv.mean[1];
        float dw = d[2] * lv.std[2] + lv.mean[2];
        float dh = d[3] * lv.std[3] + lv.mean[3];
        const float px = (x1 + x2) * 0.5f, py = (y1 + y2) * 0.5f;
        const float pw = x2 - x1, ph = y2 - y1;
        const float dxw = pw * dx, dyh = ph * dy;
        dw = fminf(fmaxf(dw, -lv.max_ratio), lv.max_ratio);
        dh = fminf(fmaxf(dh, -lv.max_ratio), lv.max_ratio);
        const float gw = pw * expf(dw), gh = ph * expf(dh);
        const float gx = px + dxw, gy = py + dyh;
        store_candidate(t, b, c, gx - gw * 0.5f, gy - gh * 0.5f, gx + gw * 0.5f, gy + gh * 0.5f, s, s > lv.score_thr, max_shape,
                        scale, boxes, scores, labels, valid, n_valid);
    }
}

// ---------------------------------------------------------------------------------------------------------------- loss
struct DenseGeom {
    int L, A, C, B, n, cls_stride, reg_stride;
    int h[BRCNN_MAX_LEVELS], w[BRCNN_MAX_LEVELS], sw[BRCNN_MAX_LEVELS], sh[BRCNN_MAX_LEVELS];
    int start[BRCNN_MAX_LEVELS + 1];        // first anchor of each level within an image
    long long row0[BRCNN_MAX_LEVELS + 1];   // first row of each level in cls / reg
    int blk0[DL_SEGS + 1];                  // first workgroup of each (level, term) pair
    const float* base[BRCNN_MAX_LEVELS];
    int gt_off[BRCNN_MAX_IMAGES + 1];
    float gamma, alpha, pos_weight, beta, mean[4], std[4];
};

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

// what one element of a head output row belongs to
struct Elem {
    int b, a, gi;
    long long cell;
    bool pos;
};

__device__ __forceinline__ Elem locate(const DenseGeom& g, const int* __restrict__ gt_inds, int l, long long r, int a) {
    Elem o;
    const int hw = g.h[l] * g.w[l];
    o.b = (int)(r / hw);
    o.cell = r - (long long)o.b * hw;
    o.a = a;
    o.gi = gt_inds[(size_t)o.b * g.n + g.start[l] + o.cell * g.A + a];
    o.pos = o.gi > 0 && o.gi <= g.gt_off[o.b + 1] - g.gt_off[o.b];
    return o;
}

// component k of bbox2delta(anchor, gt) (delta_xywh_bbox_coder.py:99-141)
__device__ __forceinline__ float delta_target(const DenseGeom& g, const float* __restrict__ gts, int l, const Elem& o, int k) {
    const int cx = (int)(o.cell % g.w[l]), cy = (int)(o.cell / g.w[l]);
    const float sx = (float)(cx * g.sw[l]), sy = (float)(cy * g.sh[l]);
    const float4 ba = *reinterpret_cast<const float4*>(g.base[l] + o.a * 4);
    const float x1 = ba.x + sx, y1 = ba.y + sy, x2 = ba.z + sx, y2 = ba.w + sy;
    const float4 gt = *reinterpret_cast<const float4*>(gts + (size_t)(g.gt_off[o.b] + o.gi - 1) * 4);
    const float pw = x2 - x1, ph = y2 - y1;
    float t;
    if (k == 0) t = ((gt.x + gt.z) * 0.5f - (x1 + x2) * 0.5f) / pw;
    else if (k == 1) t = ((gt.y + gt.w) * 0.5f - (y1 + y2) * 0.5f) / ph;
    else if (k == 2) t = logf((gt.z - gt.x) / pw);
    else t = logf((gt.w - gt.y) / ph);
    return (t - g.mean[k]) / g.std[k];
}

__device__ __forceinline__ int level_of_row(const DenseGeom& g, long long row) {
    int l = 0;
#pragma unroll
    for (int i = 1; i < BRCNN_MAX_LEVELS; i++)
        if (i < g.L && row >= g.row0[i]) l = i;
    return l;
}

// positives per image (gt_inds > 0 with a ground truth behind it): one workgroup per image
__global__ __launch_bounds__(256) void dense_count_kernel(const DenseGeom g, const int* __restrict__ gt_inds,
                                                         int* __restrict__ npos) {
    __shared__ int red[DL_THREADS];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int G = g.gt_off[b + 1] - g.gt_off[b];
    int c = 0;
    for (int i = tid; i < g.n; i += DL_THREADS) {
        const int gi = gt_inds[(size_t)b * g.n + i];
        c += (gi > 0 && gi <= G) ? 1 : 0;
    }
    red[tid] = c;
    __syncthreads();
    for (int d = DL_THREADS / 2; d > 0; d >>= 1) {
        if (tid < d) red[tid] += red[tid + d];
        __syncthreads();
    }
    if (tid == 0) npos[b] = red[0];
}

__global__ __launch_bounds__(256) void dense_loss_forward_kernel(const DenseGeom g, const float* __restrict__ cls,
                                                                const float* __restrict__ reg,
                                                                const int* __restrict__ gt_inds,
                                                                const float* __restrict__ gts,
                                                                const int64_t* __restrict__ gt_labels,
                                                                float* __restrict__ partials) {
    __shared__ float red[DL_THREADS];
    const int blk = blockIdx.x, tid = threadIdx.x;
    int seg = 0;
#pragma unroll
    for (int i = 1; i < DL_SEGS; i++)
        if (i < 2 * g.L && blk >= g.blk0[i]) seg = i;
    const int l = seg >> 1;
    const bool box = seg & 1;
    const int per_row = box ? 4 * g.A : g.A * g.C;
    const long long total = (long long)g.B * g.h[l] * g.w[l] * per_row;
    const long long e0 = (long long)(blk - g.blk0[seg]) * DL_CHUNK;
    float acc = 0.f;
    for (int j = 0; j < DL_PER_THREAD; j++) {
        const long long e = e0 + (long long)j * DL_THREADS + tid;
        if (e >= total) break;
        const long long r = e / per_row;
        const int ch = (int)(e - r * per_row);
        if (!box) {
            const int a = ch / g.C, c = ch - a * g.C;
            const Elem o = locate(g, gt_inds, l, r, a);
            if (o.gi < 0 || (o.gi > 0 && !o.pos)) continue;         // ignored or outside: label weight 0
            const bool hit = o.pos && gt_labels[g.gt_off[o.b] + o.gi - 1] == c;
            const float wt = (o.pos && g.pos_weight > 0.f) ? g.pos_weight : 1.f;
            acc += wt * focal_elem<false>(cls[(size_t)(g.row0[l] + r) * g.cls_stride + ch], hit, g.gamma, g.alpha);
        } else {
            const int a = ch >> 2, k = ch & 3;
            const Elem o = locate(g, gt_inds, l, r, a);
            if (!o.pos) continue;
            const float d = fabsf(reg[(size_t)(g.row0[l] + r) * g.reg_stride + ch] - delta_target(g, gts, l, o, k));
            acc += (g.beta > 0.f && d < g.beta) ? 0.5f * d * d / g.beta : d - 0.5f * g.beta;
        }
    }
    red[tid] = acc;
    __syncthreads();
    for (int d = DL_THREADS / 2; d > 0; d >>= 1) {
        if (tid < d) red[tid] += red[tid + d];
        __syncthreads();
    }
    if (tid == 0) partials[blk] = red[0];
}

// losses (2, L) = loss_weight / num_total_pos * the per-(level, term) sums of the partials; coef3 = the two scale
// factors for the backward pass and num_total_pos
__global__ __launch_bounds__(256) void dense_loss_finalize_kernel(const DenseGeom g, const float* __restrict__ partials,
                                                                 const int* __restrict__ npos, float lw_cls, float lw_bbox,
                                                                 float* __restrict__ losses, float* __restrict__ coef3) {
    __shared__ float red[DL_THREADS];
    __shared__ float sums[DL_SEGS];
    const int tid = threadIdx.x;
    for (int seg = 0; seg < 2 * g.L; seg++) {
        float s = 0.f;
        for (int i = g.blk0[seg] + tid; i < g.blk0[seg + 1]; i += DL_THREADS) s += partials[i];
        red[tid] = s;
        __syncthreads();
        for (int d = DL_THREADS / 2; d > 0; d >>= 1) {
            if (tid < d) red[tid] += red[tid + d];
            __syncthreads();
        }
        if (tid == 0) sums[seg] = red[0];
        __syncthreads();
    }
    if (tid == 0) {
        int total = 0;
        for (int b = 0; b < g.B; b++) total += npos[b] > 1 ? npos[b] : 1;
        const float inv = 1.f / (float)total;
        const float kc = lw_cls * inv, kb = lw_bbox * inv;
        for (int l = 0; l < g.L; l++) {
            losses[l] = sums[2 * l] * kc;
            losses[g.L + l] = sums[2 * l + 1] * kb;
        }
        coef3[0] = kc;
        coef3[1] = kb;
        coef3[2] = (float)total;
    }
}

// one thread per element of dcls (BOX = false) or dreg (BOX = true), padding columns included: every element is written
template <bool BOX>
__global__ __launch_bounds__(256) void dense_loss_backward_kernel(const DenseGeom g, const float* __restrict__ y,
                                                                 const int* __restrict__ gt_inds,
                                                                 const float* __restrict__ gts,
                                                                 const int64_t* __restrict__ gt_labels,
                                                                 const float* __restrict__ g2,
                                                                 const float* __restrict__ coef3, float* __restrict__ dy) {
    const int stride = BOX ? g.reg_stride : g.cls_stride;
    const int per_row = BOX ? 4 * g.A : g.A * g.C;
    const long long total = g.row0[g.L] * stride;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
        const long long row = e / stride;
        const int ch = (int)(e - row * stride);
        float v = 0.f;
        if (ch < per_row) {
            const int l = level_of_row(g, row);
            const long long r = row - g.row0[l];
            if (!BOX) {
                const int a = ch / g.C, c = ch - a * g.C;
                const Elem o = locate(g, gt_inds, l, r, a);
                if (!(o.gi < 0 || (o.gi > 0 && !o.pos))) {
                    const bool hit = o.pos && gt_labels[g.gt_off[o.b] + o.gi - 1] == c;
                    const float wt = (o.pos && g.pos_weight > 0.f) ? g.pos_weight : 1.f;
                    v = g2[l] * coef3[0] * (wt * focal_elem<true>(y[e], hit, g.gamma, g.alpha));
                }
            } else {
                const int a = ch >> 2, k = ch & 3;
                const Elem o = locate(g, gt_inds, l, r, a);
                if (o.pos) {
                    const float diff = y[e] - delta_target(g, gts, l, o, k);
                    const float d = fabsf(diff);
                    float gk;
                    if (g.beta > 0.f && d < g.beta) gk = diff / g.beta;
                    else gk = diff > 0.f ? 1.f : (diff < 0.f ? -1.f : 0.f);
                    v = g2[g.L + l] * coef3[1] * gk;
                }
            }
        }
        dy[e] = v;
    }
}

// cfg14_host: [focal gamma, focal alpha, pos_weight (<= 0: 1), smooth_l1_beta (0: L1), means x4, stds x4,
// loss_weight_cls, loss_weight_bbox]
int fill_geom(DenseGeom& g, int cls_stride, int reg_stride, int batch, int num_levels, const int* heights,
              const int* widths, const int* strides_w, const int* strides_h, const float* const* base_anchors, int A, int C,
              const int* gt_offsets_host, const float* cfg) {
    if (batch <= 0 || batch > BRCNN_MAX_IMAGES || num_levels <= 0 || num_levels > BRCNN_MAX_LEVELS || A <= 0 || C <= 0 ||
        !heights || !widths || !cfg || (long long)A * C > 0x7fffffLL || cls_stride < A * C || reg_stride < 4 * A)
        return BRCNN_EINVAL;
    g.L = num_levels; g.A = A; g.C = C; g.B = batch; g.cls_stride = cls_stride; g.reg_stride = reg_stride;
    long long anchors = 0, rows = 0, blocks = 0;
    for (int l = 0; l < num_levels; l++) {
        if (heights[l] <= 0 || widths[l] <= 0) return BRCNN_EINVAL;
        g.h[l] = heights[l]; g.w[l] = widths[l];
        g.sw[l] = strides_w ? strides_w[l] : 0; g.sh[l] = strides_h ? strides_h[l] : 0;
        g.base[l] = base_anchors ? base_anchors[l] : nullptr;
        g.start[l] = (int)anchors;
        g.row0[l] = rows;
        const long long cells = (long long)batch * heights[l] * widths[l];
        anchors += (long long)heights[l] * widths[l] * A;
        rows += cells;
        g.blk0[2 * l] = (int)blocks;
        blocks += (cells * A * C + DL_CHUNK - 1) / DL_CHUNK;
        g.blk0[2 * l + 1] = (int)blocks;
        blocks += (cells * A * 4 + DL_CHUNK - 1) / DL_CHUNK;
        if (anchors > 0x7fffffffLL || blocks > 0x7fffffffLL) return BRCNN_EINVAL;
    }
    for (int l = num_levels; l < BRCNN_MAX_LEVELS; l++) {
        g.h[l] = g.w[l] = 1; g.sw[l] = g.sh[l] = 0; g.base[l] = nullptr;
    }
    for (int l = num_levels; l <= BRCNN_MAX_LEVELS; l++) { g.start[l] = (int)anchors; g.row0[l] = rows; }
    for (int s = 2 * num_levels; s <= DL_SEGS; s++) g.blk0[s] = (int)blocks;
    g.n = (int)anchors;
    for (int b = 0; b <= BRCNN_MAX_IMAGES; b++) g.gt_off[b] = 0;
    if (gt_offsets_host) {
        for (int b = 0; b <= batch; b++) {
            if (gt_offsets_host[b] < 0 || (b > 0 && gt_offsets_host[b] < gt_offsets_host[b - 1])) return BRCNN_EINVAL;
            g.gt_off[b] = gt_offsets_host[b];
        }
        for (int b = batch + 1; b <= BRCNN_MAX_IMAGES; b++) g.gt_off[b] = gt_offsets_host[batch];
    }
    g.gamma = cfg[0]; g.alpha = cfg[1]; g.pos_weight = cfg[2]; g.beta = cfg[3];
    for (int i = 0; i < 4; i++) {
        g.mean[i] = cfg[4 + i]; g.std[i] = cfg[8 + i];
        if (!(g.std[i] > 0.f)) return BRCNN_EINVAL;
    }
    if (g.beta < 0.f || g.gamma < 0.f) return BRCNN_EINVAL;
    return 0;
}

bool geom_inputs_ok(const DenseGeom& g, const int* strides_w, const int* strides_h, const float* const* base_anchors,
                    const int* gt_offsets_host) {
    if (!strides_w || !strides_h || !base_anchors || !gt_offsets_host) return false;
    for (int l = 0; l < g.L; l++)
        if (!base_anchors[l]) return false;
    return true;
}

inline size_t loss_workspace_bytes(const DenseGeom& g) {
    return ((size_t)g.blk0[DL_SEGS] + (size_t)g.B) * 4;
}

}  // namespace

BRCNN_API int brcnn_dense_score(const float* cls, float* score, int64_t rows, int num_anchors, int num_classes,
                                int cls_stride, void* stream) {
    if (rows < 0 || num_anchors <= 0 || num_classes <= 0 || (long long)num_anchors * num_classes > 0x7fffffLL ||
        cls_stride < num_anchors * num_classes)
        return BRCNN_EINVAL;
    if (rows == 0) return 0;
    if (!cls || !score) return BRCNN_EINVAL;
    long long g = (rows * num_anchors + 255) / 256;
    if (g > 4096) g = 4096;
    hipLaunchKernelGGL(dense_score_kernel, dim3((int)g), dim3(256), 0, (hipStream_t)stream, cls, score, (long long)rows,
                       num_anchors, num_classes, cls_stride);
    BRCNN_LAUNCH_CHECK();
    return 0;
}

BRCNN_API int brcnn_dense_decode_levels(const int64_t* const* topk_inds, const float* const* cls, const int* cls_strides,
                                        const float* const* bbox_pred, const int* pred_strides,
                                        const float* const* base_anchors, int batch, int num_levels, const int* counts,
                                        const int* heights, const int* widths, int num_anchors, int num_classes,
                                        const int* strides_w, const int* strides_h, const float* max_shape,
                                        const float* scale_factor, const float* means4_host, const float* stds4_host,
                                        double wh_ratio_clip, float score_thr, float* boxes, float* scores,
                                        int64_t* labels, uint8_t* valid, int32_t* n_valid, void* stream) {
    if (batch < 0 || num_levels <= 0 || num_levels > BRCNN_MAX_LEVELS || num_anchors <= 0 || num_classes <= 0 ||
        (long long)num_anchors * num_classes > 0x7fffffLL || !topk_inds || !cls || !cls_strides || !bbox_pred ||
        !pred_strides || !base_anchors || !counts || !heights || !widths || !strides_w || !strides_h || !max_shape ||
        !means4_host || !stds4_host || !(wh_ratio_clip > 0.0) || !boxes || !scores || !labels || !valid || !n_valid)
        return BRCNN_EINVAL;
    DenseDecode lv = {};
    lv.num = num_levels; lv.A = num_anchors; lv.C = num_classes;
    long long T = 0;
    for (int l = 0; l < num_levels; l++) {
        if (counts[l] <= 0 || heights[l] <= 0 || widths[l] <= 0 || cls_strides[l] < num_anchors * num_classes ||
            pred_strides[l] < 4 * num_anchors || !topk_inds[l] || !cls[l] || !bbox_pred[l] || !base_anchors[l] ||
            (long long)heights[l] * widths[l] * num_anchors > 0x7fffffffLL ||
            counts[l] > (long long)heights[l] * widths[l] * num_anchors)
            return BRCNN_EINVAL;
        lv.inds[l] = topk_inds[l]; lv.cls[l] = cls[l]; lv.reg[l] = bbox_pred[l]; lv.base[l] = base_anchors[l];
        lv.cls_stride[l] = cls_strides[l]; lv.reg_stride[l] = pred_strides[l];
        lv.hw[l] = heights[l] * widths[l]; lv.width[l] = widths[l];
        lv.stride_w[l] = strides_w[l]; lv.stride_h[l] = strides_h[l];
        lv.col0[l] = (int)T;
        T += counts[l];
        if (T * num_classes > 0x7fffffffLL) return BRCNN_EINVAL;
    }
    for (int l = num_levels; l <= BRCNN_MAX_LEVELS; l++) lv.col0[l] = (int)T;
    lv.T = (int)T;
    for (int i = 0; i < 4; i++) { lv.mean[i] = means4_host[i]; lv.std[i] = stds4_host[i]; }
    lv.max_ratio = (float)fabs(log(wh_ratio_clip));
    lv.score_thr = score_thr;
    if (batch == 0) return 0;
    BRCNN_HIP_CHECK(hipMemsetAsync(n_valid, 0, sizeof(int32_t) * batch, (hipStream_t)stream));
    const long long total = (long long)batch * T * num_classes;
    long long g = (total + 255) / 256;
    if (g > 4096) g = 4096;
    hipLaunchKernelGGL(dense_decode_levels_kernel, dim3((int)g), dim3(256), 0, (hipStream_t)stream, lv, batch, max_shape,
                       scale_factor, boxes, scores, labels, valid, n_valid);
    BRCNN_LAUNCH_CHECK();
    return 0;
}

BRCNN_API size_t brcnn_dense_loss_workspace_bytes(int batch, int num_levels, const int* heights, const int* widths,
                                                  int anchors_per_cell, int num_classes) {
    DenseGeom g;
    const float cfg[14] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f};
    if (anchors_per_cell <= 0 || num_classes <= 0 || (long long)anchors_per_cell * num_classes > 0x7fffffLL) return 0;
    if (fill_geom(g, anchors_per_cell * num_classes, 4 * anchors_per_cell, batch, num_levels, heights, widths, nullptr,
                  nullptr, nullptr, anchors_per_cell, num_classes, nullptr, cfg))
        return 0;
    return loss_workspace_bytes(g);
}

BRCNN_API int brcnn_dense_loss_forward(const float* cls, int cls_stride, const float* reg, int reg_stride, int batch,
                                       int num_levels, const int* heights, const int* widths, const int* strides_w,
                                       const int* strides_h, const float* const* base_anchors, int anchors_per_cell,
                                       int num_classes, const int32_t* gt_inds, const float* gts, const int64_t* gt_labels,
                                       const int* gt_offsets_host, const float* cfg14_host, void* workspace,
                                       size_t workspace_bytes, void* stream) {
    DenseGeom g;
    const int st = fill_geom(g, cls_stride, reg_stride, batch, num_levels, heights, widths, strides_w, strides_h,
                             base_anchors, anchors_per_cell, num_classes, gt_offsets_host, cfg14_host);
    if (st) return st;
    if (!geom_inputs_ok(g, strides_w, strides_h, base_anchors, gt_offsets_host) || !cls || !reg || !gt_inds || !workspace ||
        ((!gts || !gt_labels) && g.gt_off[batch] > 0) || workspace_bytes < loss_workspace_bytes(g))
        return BRCNN_EINVAL;
    float* partials = (float*)workspace;
    int* npos = (int*)workspace + g.blk0[DL_SEGS];
    hipLaunchKernelGGL(dense_count_kernel, dim3(batch), dim3(DL_THREADS), 0, (hipStream_t)stream, g, gt_inds, npos);
    BRCNN_LAUNCH_CHECK();
    hipLaunchKernelGGL(dense_loss_forward_kernel, dim3(g.blk0[DL_SEGS]), dim3(DL_THREADS), 0, (hipStream_t)stream, g, cls,
                       reg, gt_inds, gts, gt_labels, partials);
    BRCNN_LAUNCH_CHECK();
    return 0;
}

BRCNN_API int brcnn_dense_loss_finalize(const void* workspace, size_t workspace_bytes, int batch, int num_levels,
                                        const int* heights, const int* widths, int anchors_per_cell, int num_classes,
                                        const float* cfg14_host, float* losses, float* coef3, void* stream) {
    DenseGeom g;
    if (!cfg14_host || anchors_per_cell <= 0 || num_classes <= 0 ||
        (long long)anchors_per_cell * num_classes > 0x7fffffLL)
        return BRCNN_EINVAL;
    const int st = fill_geom(g, anchors_per_cell * num_classes, 4 * anchors_per_cell, batch, num_levels, heights, widths,
                             nullptr, nullptr, nullptr, anchors_per_cell, num_classes, nullptr, cfg14_host);
    if (st) return st;
    if (!workspace || !losses || !coef3 || workspace_bytes < loss_workspace_bytes(g)) return BRCNN_EINVAL;
    const float* partials = (const float*)workspace;
    const int* npos = (const int*)workspace + g.blk0[DL_SEGS];
    hipLaunchKernelGGL(dense_loss_finalize_kernel, dim3(1), dim3(DL_THREADS), 0, (hipStream_t)stream, g, partials, npos,
                       cfg14_host[12], cfg14_host[13], losses, coef3);
    BRCNN_LAUNCH_CHECK();
    return 0;
}

BRCNN_API int brcnn_dense_loss_backward(const float* cls, int cls_stride, const float* reg, int reg_stride, int batch,
                                        int num_levels, const int* heights, const int* widths, const int* strides_w,
                                        const int* strides_h, const float* const* base_anchors, int anchors_per_cell,
                                        int num_classes, const int32_t* gt_inds, const float* gts, const int64_t* gt_labels,
                                        const int* gt_offsets_host, const float* cfg14_host, const float* grad_losses,
                                        const float* coef3, float* dcls, float* dreg, void* stream) {
    DenseGeom g;
    const int st = fill_geom(g, cls_stride, reg_stride, batch, num_levels, heights, widths, strides_w, strides_h,
                             base_anchors, anchors_per_cell, num_classes, gt_offsets_host, cfg14_host);
    if (st) return st;
    if (!geom_inputs_ok(g, strides_w, strides_h, base_anchors, gt_offsets_host) || !cls || !reg || !gt_inds ||
        !grad_losses || !coef3 || !dcls || !dreg || ((!gts || !gt_labels) && g.gt_off[batch] > 0))
        return BRCNN_EINVAL;
    const long long rows = g.row0[g.L];
    long long gc = (rows * cls_stride + 255) / 256, gr = (rows * reg_stride + 255) / 256;
    if (gc > 8192) gc = 8192;
    if (gr > 8192) gr = 8192;
    hipLaunchKernelGGL(dense_loss_backward_kernel<false>, dim3((int)gc), dim3(256), 0, (hipStream_t)stream, g, cls, gt_inds,
                       gts, gt_labels, grad_losses, coef3, dcls);
    BRCNN_LAUNCH_CHECK();
    hipLaunchKernelGGL(dense_loss_backward_kernel<true>, dim3((int)gr), dim3(256), 0, (hipStream_t)stream, g, reg, gt_inds,
                       gts, gt_labels, grad_losses, coef3, dreg);
    BRCNN_LAUNCH_CHECK();
    return 0;
}
