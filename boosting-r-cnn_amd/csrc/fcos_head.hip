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
#include "head_loss.h"

namespace {

constexpr int FC_THREADS = 256;
constexpr int FC_PER_THREAD = 8;
constexpr int FC_CHUNK = FC_THREADS * FC_PER_THREAD;        // elements (class term) or points (point terms) per workgroup
constexpr int FC_SEGS = 2 * BRCNN_MAX_LEVELS;               // (level, term): 2 * l = class term, 2 * l + 1 = point terms
constexpr float FC_INF = 1e8f;

struct FcosLayout {
    int sa, cls_off, sr, reg_off, ctr_in_r, ctr_off, norm_on_bbox, giou;
};

struct FcosGeom {
    int L, C, B, n;                         // n: points per image
    int h[BRCNN_MAX_LEVELS], w[BRCNN_MAX_LEVELS], stride[BRCNN_MAX_LEVELS];
    int start[BRCNN_MAX_LEVELS + 1];        // first point of each level within an image
    long long row0[BRCNN_MAX_LEVELS + 1];   // first row of each level in A / R
    int blk0[FC_SEGS + 1];                  // first workgroup of each (level, term) pair
    int pblk0[BRCNN_MAX_LEVELS + 1];        // first workgroup of each level in the backward pass over the points
    int gt_off[BRCNN_MAX_IMAGES + 1];
    FcosLayout lay;
    float gamma, alpha, eps_overlap, eps_loss, lw_cls, lw_bbox, lw_ctr;
};

__device__ __forceinline__ const float* ctr_ptr(const FcosLayout& y, const float* a, const float* r, size_t row) {
    return y.ctr_in_r ? r + row * y.sr + y.ctr_off : a + row * y.sa + y.ctr_off;
}

// ------------------------------------------------------------------------------------------------------------ test time
__global__ __launch_bounds__(256) void fcos_score_kernel(const float* __restrict__ a, const float* __restrict__ r,
                                                        const FcosLayout lay, int C, long long rows,
                                                        float* __restrict__ score) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < rows; i += (long long)gridDim.x * blockDim.x) {
        const float* x = a + (size_t)i * lay.sa + lay.cls_off;
        const float ct = sigmoidf_(*ctr_ptr(lay, a, r, (size_t)i));
        float m = sigmoidf_(x[0]) * ct;
        for (int c = 1; c < C; c++) m = fmaxf(m, sigmoidf_(x[c]) * ct);
        score[i] = m;
    }
}

struct FcosDecode {
    int num, C, T;
    const int64_t* inds[BRCNN_MAX_LEVELS];
    int hw[BRCNN_MAX_LEVELS], width[BRCNN_MAX_LEVELS], stride[BRCNN_MAX_LEVELS], col0[BRCNN_MAX_LEVELS + 1];
    long long row0[BRCNN_MAX_LEVELS];
    FcosLayout lay;
    float score_thr;
};

__global__ __launch_bounds__(256) void fcos_decode_levels_kernel(const FcosDecode lv, int batch, const float* __restrict__ a,
                                                                const float* __restrict__ r,
                                                                const float* __restrict__ scales,
                                                                const float* __restrict__ max_shape,
                                                                const float* __restrict__ scale_factor,
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
        long long cell = lv.inds[l][(size_t)b * count + (col - lv.col0[l])];
        cell = cell < 0 ? 0 : (cell >= lv.hw[l] ? lv.hw[l] - 1 : cell);     // (a picked index is a point of the level)
        const size_t row = (size_t)(lv.row0[l] + (long long)b * lv.hw[l] + cell);
        const float s = sigmoidf_(a[row * lv.lay.sa + lv.lay.cls_off + c]);
        const float ct = sigmoidf_(*ctr_ptr(lv.lay, a, r, row));
        const int st = lv.stride[l];
        const float px = (float)((int)(cell % lv.width[l]) * st + st / 2);
        const float py = (float)((int)(cell / lv.width[l]) * st + st / 2);
        const float* raw = r + row * lv.lay.sr + lv.lay.reg_off;
        const float sc = scales[l];
        float d[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const float v = sc * raw[k];
            d[k] = lv.lay.norm_on_bbox ? fmaxf(v, 0.f) * (float)st : expf(v);
        }
        float ox1 = px - d[0], oy1 = py - d[1], ox2 = px + d[2], oy2 = py + d[3];
        const float mh = max_shape[2 * b], mw = max_shape[2 * b + 1];
        ox1 = ox1 < 0.f ? 0.f : ox1; ox1 = ox1 > mw ? mw : ox1;
        oy1 = oy1 < 0.f ? 0.f : oy1; oy1 = oy1 > mh ? mh : oy1;
        ox2 = ox2 < 0.f ? 0.f : ox2; ox2 = ox2 > mw ? mw : ox2;
        oy2 = oy2 < 0.f ? 0.f : oy2; oy2 = oy2 > mh ? mh : oy2;
        if (scale_factor) {
            const float* sf = scale_factor + 4 * b;
            ox1 = ox1 / sf[0]; oy1 = oy1 / sf[1]; ox2 = ox2 / sf[2]; oy2 = oy2 / sf[3];
        }
        *reinterpret_cast<float4*>(boxes + (size_t)t * 4) = make_float4(ox1, oy1, ox2, oy2);
        scores[t] = s * ct;
        labels[t] = c;
        const bool ok = s > lv.score_thr;       // the class score alone: multiclass_nms masks before it applies the factor
        valid[t] = ok ? 1 : 0;
        // an integer count, one atomic per wave and image (see dense_decode_levels_kernel)
        const unsigned long long active = __ballot(1);
        const int first = __ffsll((long long)active) - 1;
        const int b_first = __shfl(b, first, WAVE);
        const unsigned long long same = __ballot(ok && b == b_first);
        if ((int)(threadIdx.x & (WAVE - 1)) == first && same) atomicAdd(n_valid + b_first, __popcll(same));
        if (ok && b != b_first) atomicAdd(n_valid + b, 1);
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

__device__ __forceinline__ int level_of_row(const FcosGeom& g, long long row) {
    int l = 0;
#pragma unroll
    for (int i = 1; i < BRCNN_MAX_LEVELS; i++)
        if (i < g.L && row >= g.row0[i]) l = i;
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

__device__ __forceinline__ Point locate(const FcosGeom& g, const int* __restrict__ gt_inds, const float* __restrict__ gts,
                                        int l, long long r, bool want_targets) {
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
__device__ __forceinline__ float box_term(const FcosGeom& g, const Point& o, const float* __restrict__ raw, float scale,
                                          float* __restrict__ dscaled) {
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

__device__ __forceinline__ float block_sum(float v, float* red, int tid) {
    __syncthreads();
    red[tid] = v;
    __syncthreads();
    for (int d = FC_THREADS / 2; d > 0; d >>= 1) {
        if (tid < d) red[tid] += red[tid + d];
        __syncthreads();
    }
    return red[0];
}

// partials: 4 arrays of `nblk` floats.  A class workgroup writes [sum, 0, 0, 0]; a point workgroup [box sum, centerness
// BCE sum, sum of the centerness targets, number of positives]
__global__ __launch_bounds__(256) void fcos_loss_forward_kernel(const FcosGeom g, const float* __restrict__ a,
                                                               const float* __restrict__ r,
                                                               const float* __restrict__ scales,
                                                               const int* __restrict__ gt_inds,
                                                               const float* __restrict__ gts,
                                                               const int64_t* __restrict__ gt_labels,
                                                               float* __restrict__ partials) {
    __shared__ float red[FC_THREADS];
    const int blk = blockIdx.x, tid = threadIdx.x, nblk = g.blk0[FC_SEGS];
    int seg = 0;
#pragma unroll
    for (int i = 1; i < FC_SEGS; i++)
        if (i < 2 * g.L && blk >= g.blk0[i]) seg = i;
    const int l = seg >> 1;
    const bool points = seg & 1;
    const long long rows = (long long)g.B * g.h[l] * g.w[l];
    const long long total = points ? rows : rows * g.C;
    const long long e0 = (long long)(blk - g.blk0[seg]) * FC_CHUNK;
    float acc0 = 0.f, acc1 = 0.f, acc2 = 0.f, acc3 = 0.f;
    for (int j = 0; j < FC_PER_THREAD; j++) {
        const long long e = e0 + (long long)j * FC_THREADS + tid;
        if (e >= total) break;
        if (!points) {
            const long long rr = e / g.C;
            const int c = (int)(e - rr * g.C);
            const Point o = locate(g, gt_inds, gts, l, rr, false);
            const bool hit = o.gi >= 0 && gt_labels[o.gi] == c;
            acc0 += focal_elem<false>(a[(size_t)(g.row0[l] + rr) * g.lay.sa + g.lay.cls_off + c], hit, g.gamma, g.alpha);
        } else {
            const Point o = locate(g, gt_inds, gts, l, e, true);
            if (o.gi < 0) continue;
            const size_t row = (size_t)(g.row0[l] + e);
            acc0 += box_term<false>(g, o, r + row * g.lay.sr + g.lay.reg_off, scales[l], nullptr) * o.ctr_t;
            acc1 += bce_logits(*ctr_ptr(g.lay, a, r, row), o.ctr_t);
            acc2 += o.ctr_t;
            acc3 += 1.f;
        }
    }
    const float s0 = block_sum(acc0, red, tid), s1 = block_sum(acc1, red, tid), s2 = block_sum(acc2, red, tid),
                s3 = block_sum(acc3, red, tid);
    if (tid == 0) {
        partials[blk] = s0;
        partials[nblk + blk] = s1;
        partials[2 * nblk + blk] = s2;
        partials[3 * nblk + blk] = s3;
    }
}

// the sum of partials[which] over the workgroups of term `term` (0 class, 1 points) of every level, level by level
__device__ __forceinline__ float term_sum(const FcosGeom& g, const float* __restrict__ partials, int which, int term,
                                          float* red, int tid) {
    const int nblk = g.blk0[FC_SEGS];
    float total = 0.f;
    for (int l = 0; l < g.L; l++) {
        const int seg = 2 * l + term;
        float s = 0.f;
        for (int i = g.blk0[seg] + tid; i < g.blk0[seg + 1]; i += FC_THREADS) s += partials[which * nblk + i];
        total += block_sum(s, red, tid);
    }
    return total;
}

// norm2 = [number of positives of the batch, sum of their centerness targets]
__global__ __launch_bounds__(256) void fcos_loss_norm_kernel(const FcosGeom g, const float* __restrict__ partials,
                                                            float* __restrict__ norm2) {
    __shared__ float red[FC_THREADS];
    const int tid = threadIdx.x;
    const float cnt = term_sum(g, partials, 3, 1, red, tid), sum = term_sum(g, partials, 2, 1, red, tid);
    if (tid == 0) { norm2[0] = cnt; norm2[1] = sum; }
}

// losses3 = [loss_cls, loss_bbox, loss_centerness]; coef3 = [lw_cls / N, lw_bbox / S, lw_ctr / N] for the backward pass
__global__ __launch_bounds__(256) void fcos_loss_finalize_kernel(const FcosGeom g, const float* __restrict__ partials,
                                                                const float* __restrict__ norm2,
                                                                float* __restrict__ losses3, float* __restrict__ coef3) {
    __shared__ float red[FC_THREADS];
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

// one thread per element of dA (rows, stride_a), padding columns included: every element is written
__global__ __launch_bounds__(256) void fcos_loss_backward_a_kernel(const FcosGeom g, const float* __restrict__ a,
                                                                  const float* __restrict__ r,
                                                                  const int* __restrict__ gt_inds,
                                                                  const float* __restrict__ gts,
                                                                  const int64_t* __restrict__ gt_labels,
                                                                  const float* __restrict__ g3,
                                                                  const float* __restrict__ coef3, float* __restrict__ da) {
    const long long total = g.row0[g.L] * g.lay.sa;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
        const long long row = e / g.lay.sa;
        const int ch = (int)(e - row * g.lay.sa);
        const bool is_cls = ch >= g.lay.cls_off && ch < g.lay.cls_off + g.C;
        const bool is_ctr = !g.lay.ctr_in_r && ch == g.lay.ctr_off;
        float v = 0.f;
        if (is_cls || is_ctr) {
            const int l = level_of_row(g, row);
            const Point o = locate(g, gt_inds, gts, l, row - g.row0[l], is_ctr);
            if (is_cls) {
                const bool hit = o.gi >= 0 && gt_labels[o.gi] == ch - g.lay.cls_off;
                v = g3[0] * coef3[0] * focal_elem<true>(a[e], hit, g.gamma, g.alpha);
            } else if (o.gi >= 0) {
                v = g3[2] * coef3[2] * (sigmoidf_(a[e]) - o.ctr_t);
            }
        }
        da[e] = v;
    }
}

// one thread per row of dR (rows, stride_r): the 4 box columns, the centerness column under centerness_on_reg, zeros
// elsewhere; and per workgroup the partial of dscale_l = sum over the level's rows of d(scaled) * raw
__global__ __launch_bounds__(256) void fcos_loss_backward_r_kernel(const FcosGeom g, const float* __restrict__ a,
                                                                  const float* __restrict__ r,
                                                                  const float* __restrict__ scales,
                                                                  const int* __restrict__ gt_inds,
                                                                  const float* __restrict__ gts,
                                                                  const float* __restrict__ g3,
                                                                  const float* __restrict__ coef3, float* __restrict__ dr,
                                                                  float* __restrict__ dscale_partials) {
    __shared__ float red[FC_THREADS];
    const int blk = blockIdx.x, tid = threadIdx.x;
    int l = 0;
#pragma unroll
    for (int i = 1; i < BRCNN_MAX_LEVELS; i++)
        if (i < g.L && blk >= g.pblk0[i]) l = i;
    const long long rows = (long long)g.B * g.h[l] * g.w[l];
    const long long e0 = (long long)(blk - g.pblk0[l]) * FC_CHUNK;
    float acc = 0.f;
    for (int j = 0; j < FC_PER_THREAD; j++) {
        const long long e = e0 + (long long)j * FC_THREADS + tid;
        if (e >= rows) break;
        const size_t row = (size_t)(g.row0[l] + e);
        float* out = dr + row * g.lay.sr;
        const Point o = locate(g, gt_inds, gts, l, e, true);
        float ds[4] = {0.f, 0.f, 0.f, 0.f}, dc = 0.f;
        if (o.gi >= 0) {
            const float* raw = r + row * g.lay.sr + g.lay.reg_off;
            const float sc = scales[l];
            box_term<true>(g, o, raw, sc, ds);
            const float k = g3[1] * coef3[1] * o.ctr_t;
#pragma unroll
            for (int q = 0; q < 4; q++) {
                ds[q] = k * ds[q];
                acc += ds[q] * raw[q];
                ds[q] = ds[q] * sc;
            }
            if (g.lay.ctr_in_r) dc = g3[2] * coef3[2] * (sigmoidf_(r[row * g.lay.sr + g.lay.ctr_off]) - o.ctr_t);
        }
        for (int ch = 0; ch < g.lay.sr; ch++) {
            const int q = ch - g.lay.reg_off;
            out[ch] = (q >= 0 && q < 4) ? ds[q] : ((g.lay.ctr_in_r && ch == g.lay.ctr_off) ? dc : 0.f);
        }
    }
    const float s = block_sum(acc, red, tid);
    if (tid == 0) dscale_partials[blk] = s;
}

__global__ __launch_bounds__(256) void fcos_dscale_kernel(const FcosGeom g, const float* __restrict__ dscale_partials,
                                                         float* __restrict__ dscale) {
    __shared__ float red[FC_THREADS];
    const int tid = threadIdx.x;
    for (int l = 0; l < g.L; l++) {
        float s = 0.f;
        for (int i = g.pblk0[l] + tid; i < g.pblk0[l + 1]; i += FC_THREADS) s += dscale_partials[i];
        const float t = block_sum(s, red, tid);
        if (tid == 0) dscale[l] = t;
    }
}

// --------------------------------------------------------------------------------------------------------------- host
bool layout_ok(const int* v, int C) {
    if (!v) return false;
    const int sa = v[0], cls_off = v[1], sr = v[2], reg_off = v[3], ctr_in_r = v[4], ctr_off = v[5];
    if (sa <= 0 || sr <= 0 || cls_off < 0 || reg_off < 0 || ctr_off < 0 || cls_off + C > sa || reg_off + 4 > sr) return false;
    if (ctr_in_r ? (ctr_off >= sr || (ctr_off >= reg_off && ctr_off < reg_off + 4))
                 : (ctr_off >= sa || (ctr_off >= cls_off && ctr_off < cls_off + C)))
        return false;
    return true;
}

FcosLayout make_layout(const int* v) {
    FcosLayout y;
    y.sa = v[0]; y.cls_off = v[1]; y.sr = v[2]; y.reg_off = v[3]; y.ctr_in_r = v[4] != 0; y.ctr_off = v[5];
    y.norm_on_bbox = v[6] != 0; y.giou = v[7] != 0;
    return y;
}

// cfg7_host: [focal gamma, focal alpha, eps of bbox_overlaps, eps of the IoU-log clamp, loss_weight_cls, loss_weight_bbox,
// loss_weight_centerness]
int fill_geom(FcosGeom& g, int batch, int num_levels, const int* heights, const int* widths, const int* strides,
              int C, const int* gt_offsets_host, const int* layout8, const float* cfg7) {
    if (batch <= 0 || batch > BRCNN_MAX_IMAGES || num_levels <= 0 || num_levels > BRCNN_MAX_LEVELS || C <= 0 ||
        C > 0x7fffff || !heights || !widths || !strides)
        return BRCNN_EINVAL;
    g.L = num_levels; g.C = C; g.B = batch;
    long long points = 0, rows = 0, blocks = 0, pblocks = 0;
    for (int l = 0; l < num_levels; l++) {
        if (heights[l] <= 0 || widths[l] <= 0 || strides[l] <= 0 || strides[l] > 0x7fff ||
            (long long)heights[l] * strides[l] > 0x7fffffLL || (long long)widths[l] * strides[l] > 0x7fffffLL)
            return BRCNN_EINVAL;
        g.h[l] = heights[l]; g.w[l] = widths[l]; g.stride[l] = strides[l];
        g.start[l] = (int)points;
        g.row0[l] = rows;
        const long long cells = (long long)batch * heights[l] * widths[l];
        points += (long long)heights[l] * widths[l];
        rows += cells;
        g.blk0[2 * l] = (int)blocks;
        blocks += (cells * C + FC_CHUNK - 1) / FC_CHUNK;
        g.blk0[2 * l + 1] = (int)blocks;
        blocks += (cells + FC_CHUNK - 1) / FC_CHUNK;
        g.pblk0[l] = (int)pblocks;
        pblocks += (cells + FC_CHUNK - 1) / FC_CHUNK;
        if (points > 0x7fffffffLL / batch || blocks > 0x3fffffffLL) return BRCNN_EINVAL;
    }
    for (int l = num_levels; l < BRCNN_MAX_LEVELS; l++) { g.h[l] = g.w[l] = g.stride[l] = 1; }
    for (int l = num_levels; l <= BRCNN_MAX_LEVELS; l++) { g.start[l] = (int)points; g.row0[l] = rows; g.pblk0[l] = (int)pblocks; }
    for (int s = 2 * num_levels; s <= FC_SEGS; s++) g.blk0[s] = (int)blocks;
    g.n = (int)points;
    for (int b = 0; b <= BRCNN_MAX_IMAGES; b++) g.gt_off[b] = 0;
    if (gt_offsets_host) {
        for (int b = 0; b <= batch; b++) {
            if (gt_offsets_host[b] < 0 || (b > 0 && gt_offsets_host[b] < gt_offsets_host[b - 1])) return BRCNN_EINVAL;
            g.gt_off[b] = gt_offsets_host[b];
        }
        for (int b = batch + 1; b <= BRCNN_MAX_IMAGES; b++) g.gt_off[b] = gt_offsets_host[batch];
    }
    g.lay = FcosLayout{};
    if (layout8) {
        if (!layout_ok(layout8, C)) return BRCNN_EINVAL;
        g.lay = make_layout(layout8);
    }
    g.gamma = g.alpha = 0.f; g.eps_overlap = g.eps_loss = 1e-6f; g.lw_cls = g.lw_bbox = g.lw_ctr = 1.f;
    if (cfg7) {
        g.gamma = cfg7[0]; g.alpha = cfg7[1]; g.eps_overlap = cfg7[2]; g.eps_loss = cfg7[3];
        g.lw_cls = cfg7[4]; g.lw_bbox = cfg7[5]; g.lw_ctr = cfg7[6];
        if (g.gamma < 0.f || !(g.eps_overlap > 0.f) || !(g.eps_loss > 0.f)) return BRCNN_EINVAL;
    }
    return 0;
}

inline size_t loss_workspace_bytes(const FcosGeom& g) {
    // forward / finalize: 4 partial arrays; backward: one dscale partial per point workgroup (fewer)
    return (size_t)4 * (size_t)g.blk0[FC_SEGS] * sizeof(float);
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
    if (batch < 0 || num_levels <= 0 || num_levels > BRCNN_MAX_LEVELS || num_classes <= 0 ||
        num_classes > 0x7fffff || !topk_inds || !counts || !a || !r || !layout_ok(layout8_host, num_classes) || !scales ||
        !heights || !widths || !strides || !max_shape || !boxes || !scores || !labels || !valid || !n_valid)
        return BRCNN_EINVAL;
    FcosDecode lv = {};
    lv.num = num_levels; lv.C = num_classes;
    lv.lay = make_layout(layout8_host);
    long long T = 0, rows = 0;
    for (int l = 0; l < num_levels; l++) {
        if (counts[l] <= 0 || heights[l] <= 0 || widths[l] <= 0 || strides[l] <= 0 || strides[l] > 0x7fff || !topk_inds[l] ||
            (long long)heights[l] * widths[l] > 0x7fffffffLL || counts[l] > (long long)heights[l] * widths[l] ||
            (long long)heights[l] * strides[l] > 0x7fffffLL || (long long)widths[l] * strides[l] > 0x7fffffLL)
            return BRCNN_EINVAL;
        lv.inds[l] = topk_inds[l];
        lv.hw[l] = heights[l] * widths[l]; lv.width[l] = widths[l]; lv.stride[l] = strides[l];
        lv.row0[l] = rows;
        rows += (long long)batch * lv.hw[l];
        lv.col0[l] = (int)T;
        T += counts[l];
        if (T * num_classes > 0x7fffffffLL) return BRCNN_EINVAL;
    }
    for (int l = num_levels; l <= BRCNN_MAX_LEVELS; l++) lv.col0[l] = (int)T;
    lv.T = (int)T;
    lv.score_thr = score_thr;
    if (batch == 0) return 0;
    BRCNN_HIP_CHECK(hipMemsetAsync(n_valid, 0, sizeof(int32_t) * batch, (hipStream_t)stream));
    const long long total = (long long)batch * T * num_classes;
    long long g = (total + 255) / 256;
    if (g > 4096) g = 4096;
    hipLaunchKernelGGL(fcos_decode_levels_kernel, dim3((int)g), dim3(256), 0, (hipStream_t)stream, lv, batch, a, r, scales,
                       max_shape, scale_factor, boxes, scores, labels, valid, n_valid);
    BRCNN_LAUNCH_CHECK();
    return 0;
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
    const long long total = (long long)batch * g.n;
    long long grid = (total + 255) / 256;
    if (grid > 8192) grid = 8192;
    hipLaunchKernelGGL(fcos_assign_kernel, dim3((int)grid), dim3(256), 0, (hipStream_t)stream, g, as, gts, gt_inds);
    BRCNN_LAUNCH_CHECK();
    return 0;
}

BRCNN_API size_t brcnn_fcos_loss_workspace_bytes(int batch, int num_levels, const int* heights, const int* widths,
                                                 int num_classes) {
    FcosGeom g;
    int ones[BRCNN_MAX_LEVELS];
    for (int l = 0; l < BRCNN_MAX_LEVELS; l++) ones[l] = 1;
    if (fill_geom(g, batch, num_levels, heights, widths, ones, num_classes, nullptr, nullptr, nullptr)) return 0;
    return loss_workspace_bytes(g);
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
        workspace_bytes < loss_workspace_bytes(g))
        return BRCNN_EINVAL;
    float* partials = (float*)workspace;
    hipLaunchKernelGGL(fcos_loss_forward_kernel, dim3(g.blk0[FC_SEGS]), dim3(FC_THREADS), 0, (hipStream_t)stream, g, a, r,
                       scales, gt_inds, gts, gt_labels, partials);
    BRCNN_LAUNCH_CHECK();
    hipLaunchKernelGGL(fcos_loss_norm_kernel, dim3(1), dim3(FC_THREADS), 0, (hipStream_t)stream, g, partials, norm2);
    BRCNN_LAUNCH_CHECK();
    return 0;
}

BRCNN_API int brcnn_fcos_loss_finalize(const void* workspace, size_t workspace_bytes, const float* norm2, int batch,
                                       int num_levels, const int* heights, const int* widths, int num_classes,
                                       const float* cfg7_host, float* losses3, float* coef3, void* stream) {
    FcosGeom g;
    int ones[BRCNN_MAX_LEVELS];
    for (int l = 0; l < BRCNN_MAX_LEVELS; l++) ones[l] = 1;
    if (!cfg7_host) return BRCNN_EINVAL;
    const int st = fill_geom(g, batch, num_levels, heights, widths, ones, num_classes, nullptr, nullptr, cfg7_host);
    if (st) return st;
    if (!workspace || !norm2 || !losses3 || !coef3 || workspace_bytes < loss_workspace_bytes(g)) return BRCNN_EINVAL;
    hipLaunchKernelGGL(fcos_loss_finalize_kernel, dim3(1), dim3(FC_THREADS), 0, (hipStream_t)stream, g,
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
    if (!a || !r || !scales || !gt_inds || !grad_losses3 || !coef3 || !workspace || !da || !dr || !dscale ||
        ((!gts || !gt_labels) && g.gt_off[batch] > 0) || workspace_bytes < loss_workspace_bytes(g))
        return BRCNN_EINVAL;
    long long ga = (g.row0[g.L] * g.lay.sa + 255) / 256;
    if (ga > 8192) ga = 8192;
    hipLaunchKernelGGL(fcos_loss_backward_a_kernel, dim3((int)ga), dim3(256), 0, (hipStream_t)stream, g, a, r, gt_inds, gts,
                       gt_labels, grad_losses3, coef3, da);
    BRCNN_LAUNCH_CHECK();
    float* dsp = (float*)workspace;
    hipLaunchKernelGGL(fcos_loss_backward_r_kernel, dim3(g.pblk0[g.L]), dim3(FC_THREADS), 0, (hipStream_t)stream, g, a, r,
                       scales, gt_inds, gts, grad_losses3, coef3, dr, dsp);
    BRCNN_LAUNCH_CHECK();
    hipLaunchKernelGGL(fcos_dscale_kernel, dim3(1), dim3(FC_THREADS), 0, (hipStream_t)stream, g, dsp, dscale);
    BRCNN_LAUNCH_CHECK();
    return 0;
}
