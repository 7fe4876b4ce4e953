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
//   atss_decode_levels : fcos_decode_levels_kernel with the anchor decode of dense_decode_levels_kernel.
//   atss_loss_*        : ATSSHead.loss, the block-partial scheme of fcos_loss_* (fixed order within a thread, LDS tree, one
//                        finalize workgroup): no float atomics, the same bits from run to run.
#include "box_iou.h"
#include "head_loss.h"

namespace {

constexpr int AT_THREADS = 256;
constexpr int AT_PER_THREAD = 8;
constexpr int AT_CHUNK = AT_THREADS * AT_PER_THREAD;        // elements (class term) or anchors (anchor terms) per workgroup
constexpr int AT_SEGS = 2 * BRCNN_MAX_LEVELS;               // (level, term): 2 * l = class term, 2 * l + 1 = anchor terms
constexpr int AT_MAX_TOPK = 16;

struct AtssLayout {
    int sa, cls_off, sr, reg_off, ctr_in_r, ctr_off;
};

struct AtssGeom {
    int L, C, B, n;                         // n: anchors per image
    int h[BRCNN_MAX_LEVELS], w[BRCNN_MAX_LEVELS], stride[BRCNN_MAX_LEVELS];
    float base[BRCNN_MAX_LEVELS][4];
    int start[BRCNN_MAX_LEVELS + 1];        // first anchor of each level within an image
    long long row0[BRCNN_MAX_LEVELS + 1];   // first row of each level in A / R
    int blk0[AT_SEGS + 1];                  // first workgroup of each (level, term) pair
    int pblk0[BRCNN_MAX_LEVELS + 1];        // first workgroup of each level in the backward pass over the anchors
    int gt_off[BRCNN_MAX_IMAGES + 1];
    AtssLayout lay;
    float gamma, alpha, eps, lw_cls, lw_bbox, lw_ctr, mean[4], std[4], max_ratio;
};

__device__ __forceinline__ const float* ctr_ptr(const AtssLayout& y, const float* a, const float* r, size_t row) {
    return y.ctr_in_r ? r + row * y.sr + y.ctr_off : a + row * y.sa + y.ctr_off;
}

__device__ __forceinline__ float4 anchor_of(const float* base, int width, int stride, int cell) {
    const float sx = (float)((cell % width) * stride), sy = (float)((cell / width) * stride);
    return make_float4(base[0] + sx, base[1] + sy, base[2] + sx, base[3] + sy);
}

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
    for (int d = AT_THREADS / 2; d > 0; d >>= 1) {
        if (tid < d && red[tid + d] < red[tid]) red[tid] = red[tid + d];
        __syncthreads();
    }
    return red[0];
}

__global__ __launch_bounds__(256) void atss_assign_kernel(const AtssGeom g, const AtssAssign as, const float* __restrict__ gts,
                                                         unsigned long long* __restrict__ keys) {
    __shared__ unsigned long long red[AT_THREADS];
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
            for (int cell = tid; cell < hw; cell += AT_THREADS) {
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
    for (int c = tid; c < m; c += AT_THREADS) {
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
    for (int c = tid; c < m; c += AT_THREADS) {
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

// ------------------------------------------------------------------------------------------------------------ test time
struct AtssDecode {
    int num, C, T;
    const int64_t* inds[BRCNN_MAX_LEVELS];
    int hw[BRCNN_MAX_LEVELS], width[BRCNN_MAX_LEVELS], stride[BRCNN_MAX_LEVELS], col0[BRCNN_MAX_LEVELS + 1];
    long long row0[BRCNN_MAX_LEVELS];
    float base[BRCNN_MAX_LEVELS][4];
    AtssLayout lay;
    float mean[4], std[4], max_ratio, score_thr;
};

__global__ __launch_bounds__(256) void atss_decode_levels_kernel(const AtssDecode lv, int batch, const float* __restrict__ a,
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
        cell = cell < 0 ? 0 : (cell >= lv.hw[l] ? lv.hw[l] - 1 : cell);     // (a picked index is an anchor of the level)
        const size_t row = (size_t)(lv.row0[l] + (long long)b * lv.hw[l] + cell);
        const float s = sigmoidf_(a[row * lv.lay.sa + lv.lay.cls_off + c]);
        const float ct = sigmoidf_(*ctr_ptr(lv.lay, a, r, row));
        const float4 an = anchor_of(lv.base[l], lv.width[l], lv.stride[l], (int)cell);
        const float* raw = r + row * lv.lay.sr + lv.lay.reg_off;
        const float sc = scales[l];
        const float d[4] = {sc * raw[0], sc * raw[1], sc * raw[2], sc * raw[3]};
        const float4 o = decode_anchor<false>(an, d, lv.mean, lv.std, lv.max_ratio, nullptr);
        float ox1 = o.x, oy1 = o.y, ox2 = o.z, oy2 = o.w;
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

// ----------------------------------------------------------------------------------------------------------------- loss
__device__ __forceinline__ int level_of_row(const AtssGeom& g, long long row) {
    int l = 0;
#pragma unroll
    for (int i = 1; i < BRCNN_MAX_LEVELS; i++)
        if (i < g.L && row >= g.row0[i]) l = i;
    return l;
}

// what one row of the head outputs is: its image, its state and, for a positive, its anchor and targets
struct Cell {
    int b, gi;          // gi: index into the packed gts (positive), -1 negative, -2 invalid (weight 0)
    float4 an, gt;      // the anchor; gt' = delta2bbox(anchor, bbox2delta(anchor, gt))
    float ctr_t;
};

__device__ __forceinline__ Cell locate(const AtssGeom& g, const int* __restrict__ gt_inds, const float* __restrict__ gts,
                                       int l, long long r, bool want_targets) {
    Cell o;
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
__device__ __forceinline__ float box_term(const AtssGeom& g, const Cell& o, const float* __restrict__ raw, float scale,
                                          float* __restrict__ dscaled) {
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

__device__ __forceinline__ float block_sum(float v, float* red, int tid) {
    __syncthreads();
    red[tid] = v;
    __syncthreads();
    for (int d = AT_THREADS / 2; d > 0; d >>= 1) {
        if (tid < d) red[tid] += red[tid + d];
        __syncthreads();
    }
    return red[0];
}

// partials: 3 arrays of `nblk` floats.  A class workgroup writes [sum, 0, 0]; an anchor workgroup [box sum, centerness BCE
// sum, sum of the centerness targets]
__global__ __launch_bounds__(256) void atss_loss_forward_kernel(const AtssGeom g, const float* __restrict__ a,
                                                               const float* __restrict__ r,
                                                               const float* __restrict__ scales,
                                                               const int* __restrict__ gt_inds,
                                                               const float* __restrict__ gts,
                                                               const int64_t* __restrict__ gt_labels,
                                                               float* __restrict__ partials) {
    __shared__ float red[AT_THREADS];
    const int blk = blockIdx.x, tid = threadIdx.x, nblk = g.blk0[AT_SEGS];
    int seg = 0;
#pragma unroll
    for (int i = 1; i < AT_SEGS; i++)
        if (i < 2 * g.L && blk >= g.blk0[i]) seg = i;
    const int l = seg >> 1;
    const bool anchors = seg & 1;
    const long long rows = (long long)g.B * g.h[l] * g.w[l];
    const long long total = anchors ? rows : rows * g.C;
    const long long e0 = (long long)(blk - g.blk0[seg]) * AT_CHUNK;
    float acc0 = 0.f, acc1 = 0.f, acc2 = 0.f;
    for (int j = 0; j < AT_PER_THREAD; j++) {
        const long long e = e0 + (long long)j * AT_THREADS + tid;
        if (e >= total) break;
        if (!anchors) {
            const long long rr = e / g.C;
            const int c = (int)(e - rr * g.C);
            const Cell o = locate(g, gt_inds, gts, l, rr, false);
            if (o.gi == -2) continue;
            const bool hit = o.gi >= 0 && gt_labels[o.gi] == c;
            acc0 += focal_elem<false>(a[(size_t)(g.row0[l] + rr) * g.lay.sa + g.lay.cls_off + c], hit, g.gamma, g.alpha);
        } else {
            const Cell o = locate(g, gt_inds, gts, l, e, true);
            if (o.gi < 0) continue;
            const size_t row = (size_t)(g.row0[l] + e);
            acc0 += box_term<false>(g, o, r + row * g.lay.sr + g.lay.reg_off, scales[l], nullptr) * o.ctr_t;
            acc1 += bce_logits(*ctr_ptr(g.lay, a, r, row), o.ctr_t);
            acc2 += o.ctr_t;
        }
    }
    const float s0 = block_sum(acc0, red, tid), s1 = block_sum(acc1, red, tid), s2 = block_sum(acc2, red, tid);
    if (tid == 0) {
        partials[blk] = s0;
        partials[nblk + blk] = s1;
        partials[2 * nblk + blk] = s2;
    }
}

// the sum of partials[which] over the workgroups of (level l, term)
__device__ __forceinline__ float level_sum(const AtssGeom& g, const float* __restrict__ partials, int which, int l, int term,
                                           float* red, int tid) {
    const int nblk = g.blk0[AT_SEGS], seg = 2 * l + term;
    float s = 0.f;
    for (int i = g.blk0[seg] + tid; i < g.blk0[seg + 1]; i += AT_THREADS) s += partials[which * nblk + i];
    return block_sum(s, red, tid);
}

// norm2 = [sum over images of max(number of positives, 1), sum of the centerness targets]; a count is an integer below
// 2^24, exact in fp32
__global__ __launch_bounds__(256) void atss_loss_norm_kernel(const AtssGeom g, const int* __restrict__ gt_inds,
                                                            const float* __restrict__ partials, float* __restrict__ norm2) {
    __shared__ float red[AT_THREADS];
    const int tid = threadIdx.x;
    float cnt = 0.f;
    for (int b = 0; b < g.B; b++) {
        const int G = g.gt_off[b + 1] - g.gt_off[b];
        float c = 0.f;
        for (int i = tid; i < g.n; i += AT_THREADS) {
            const int gi = gt_inds[(size_t)b * g.n + i];
            c += (gi > 0 && gi <= G) ? 1.f : 0.f;
        }
        cnt += fmaxf(block_sum(c, red, tid), 1.f);
    }
    float sum = 0.f;
    for (int l = 0; l < g.L; l++) sum += level_sum(g, partials, 2, l, 1, red, tid);
    if (tid == 0) { norm2[0] = cnt; norm2[1] = sum; }
}

// losses (3, L) = [loss_cls | loss_bbox | loss_centerness] per level; coef3 = [lw_cls / N, lw_bbox / S, lw_ctr / N]
__global__ __launch_bounds__(256) void atss_loss_finalize_kernel(const AtssGeom g, const float* __restrict__ partials,
                                                                const float* __restrict__ norm2,
                                                                float* __restrict__ losses, float* __restrict__ coef3) {
    __shared__ float red[AT_THREADS];
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

// one thread per element of dA (rows, stride_a), padding columns included: every element is written
__global__ __launch_bounds__(256) void atss_loss_backward_a_kernel(const AtssGeom g, const float* __restrict__ a,
                                                                  const float* __restrict__ r,
                                                                  const int* __restrict__ gt_inds,
                                                                  const float* __restrict__ gts,
                                                                  const int64_t* __restrict__ gt_labels,
                                                                  const float* __restrict__ gl,
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
            const Cell o = locate(g, gt_inds, gts, l, row - g.row0[l], is_ctr);
            if (is_cls) {
                if (o.gi != -2) {
                    const bool hit = o.gi >= 0 && gt_labels[o.gi] == ch - g.lay.cls_off;
                    v = gl[l] * coef3[0] * focal_elem<true>(a[e], hit, g.gamma, g.alpha);
                }
            } else if (o.gi >= 0) {
                v = gl[2 * g.L + l] * coef3[2] * (sigmoidf_(a[e]) - o.ctr_t);
            }
        }
        da[e] = v;
    }
}

// one thread per row of dR (rows, stride_r): the 4 delta columns, the centerness column when it rides on R, zeros elsewhere;
// and per workgroup the partial of dscale_l = sum over the level's rows of d(scaled) * raw
__global__ __launch_bounds__(256) void atss_loss_backward_r_kernel(const AtssGeom g, const float* __restrict__ a,
                                                                  const float* __restrict__ r,
                                                                  const float* __restrict__ scales,
                                                                  const int* __restrict__ gt_inds,
                                                                  const float* __restrict__ gts,
                                                                  const float* __restrict__ gl,
                                                                  const float* __restrict__ coef3, float* __restrict__ dr,
                                                                  float* __restrict__ dscale_partials) {
    __shared__ float red[AT_THREADS];
    const int blk = blockIdx.x, tid = threadIdx.x;
    int l = 0;
#pragma unroll
    for (int i = 1; i < BRCNN_MAX_LEVELS; i++)
        if (i < g.L && blk >= g.pblk0[i]) l = i;
    const long long rows = (long long)g.B * g.h[l] * g.w[l];
    const long long e0 = (long long)(blk - g.pblk0[l]) * AT_CHUNK;
    float acc = 0.f;
    for (int j = 0; j < AT_PER_THREAD; j++) {
        const long long e = e0 + (long long)j * AT_THREADS + tid;
        if (e >= rows) break;
        const size_t row = (size_t)(g.row0[l] + e);
        float* out = dr + row * g.lay.sr;
        const Cell o = locate(g, gt_inds, gts, l, e, true);
        float ds[4] = {0.f, 0.f, 0.f, 0.f}, dc = 0.f;
        if (o.gi >= 0) {
            const float* raw = r + row * g.lay.sr + g.lay.reg_off;
            const float sc = scales[l];
            box_term<true>(g, o, raw, sc, ds);
            const float k = gl[g.L + l] * coef3[1] * o.ctr_t;
#pragma unroll
            for (int q = 0; q < 4; q++) {
                ds[q] = k * ds[q];
                acc += ds[q] * raw[q];
                ds[q] = ds[q] * sc;
            }
            if (g.lay.ctr_in_r) dc = gl[2 * g.L + l] * coef3[2] * (sigmoidf_(r[row * g.lay.sr + g.lay.ctr_off]) - o.ctr_t);
        }
        for (int ch = 0; ch < g.lay.sr; ch++) {
            const int q = ch - g.lay.reg_off;
            out[ch] = (q >= 0 && q < 4) ? ds[q] : ((g.lay.ctr_in_r && ch == g.lay.ctr_off) ? dc : 0.f);
        }
    }
    const float s = block_sum(acc, red, tid);
    if (tid == 0) dscale_partials[blk] = s;
}

__global__ __launch_bounds__(256) void atss_dscale_kernel(const AtssGeom g, const float* __restrict__ dscale_partials,
                                                         float* __restrict__ dscale) {
    __shared__ float red[AT_THREADS];
    const int tid = threadIdx.x;
    for (int l = 0; l < g.L; l++) {
        float s = 0.f;
        for (int i = g.pblk0[l] + tid; i < g.pblk0[l + 1]; i += AT_THREADS) s += dscale_partials[i];
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

AtssLayout make_layout(const int* v) {
    AtssLayout y;
    y.sa = v[0]; y.cls_off = v[1]; y.sr = v[2]; y.reg_off = v[3]; y.ctr_in_r = v[4] != 0; y.ctr_off = v[5];
    return y;
}

bool level_ok(int h, int w, int stride) {
    return h > 0 && w > 0 && stride > 0 && stride <= 0x7fff && (long long)h * w <= 0x7fffffffLL &&
           (long long)h * stride <= 0x7fffffLL && (long long)w * stride <= 0x7fffffLL;
}

int fill_geom(AtssGeom& g, int batch, int num_levels, const int* heights, const int* widths, const int* strides,
              const float* base, int C, const int* gt_offsets_host, const int* layout8, const float* cfg15) {
    if (batch <= 0 || batch > BRCNN_MAX_IMAGES || num_levels <= 0 || num_levels > BRCNN_MAX_LEVELS || C <= 0 ||
        C > 0x7fffff || !heights || !widths || !strides)
        return BRCNN_EINVAL;
    g.L = num_levels; g.C = C; g.B = batch;
    long long anchors = 0, rows = 0, blocks = 0, pblocks = 0;
    for (int l = 0; l < num_levels; l++) {
        if (!level_ok(heights[l], widths[l], strides[l])) return BRCNN_EINVAL;
        g.h[l] = heights[l]; g.w[l] = widths[l]; g.stride[l] = strides[l];
        for (int k = 0; k < 4; k++) g.base[l][k] = base ? base[4 * l + k] : 0.f;
        g.start[l] = (int)anchors;
        g.row0[l] = rows;
        const long long cells = (long long)batch * heights[l] * widths[l];
        anchors += (long long)heights[l] * widths[l];
        rows += cells;
        g.blk0[2 * l] = (int)blocks;
        blocks += (cells * C + AT_CHUNK - 1) / AT_CHUNK;
        g.blk0[2 * l + 1] = (int)blocks;
        blocks += (cells + AT_CHUNK - 1) / AT_CHUNK;
        g.pblk0[l] = (int)pblocks;
        pblocks += (cells + AT_CHUNK - 1) / AT_CHUNK;
        if (anchors > 0x7fffffffLL / batch || blocks > 0x3fffffffLL) return BRCNN_EINVAL;
    }
    for (int l = num_levels; l < BRCNN_MAX_LEVELS; l++) {
        g.h[l] = g.w[l] = g.stride[l] = 1;
        for (int k = 0; k < 4; k++) g.base[l][k] = 0.f;
    }
    for (int l = num_levels; l <= BRCNN_MAX_LEVELS; l++) { g.start[l] = (int)anchors; g.row0[l] = rows; g.pblk0[l] = (int)pblocks; }
    for (int s = 2 * num_levels; s <= AT_SEGS; s++) g.blk0[s] = (int)blocks;
    g.n = (int)anchors;
    for (int b = 0; b <= BRCNN_MAX_IMAGES; b++) g.gt_off[b] = 0;
    if (gt_offsets_host) {
        for (int b = 0; b <= batch; b++) {
            if (gt_offsets_host[b] < 0 || (b > 0 && gt_offsets_host[b] < gt_offsets_host[b - 1])) return BRCNN_EINVAL;
            g.gt_off[b] = gt_offsets_host[b];
        }
        for (int b = batch + 1; b <= BRCNN_MAX_IMAGES; b++) g.gt_off[b] = gt_offsets_host[batch];
    }
    g.lay = AtssLayout{};
    if (layout8) {
        if (!layout_ok(layout8, C)) return BRCNN_EINVAL;
        g.lay = make_layout(layout8);
    }
    g.gamma = g.alpha = 0.f; g.eps = 1e-6f; g.lw_cls = g.lw_bbox = g.lw_ctr = 1.f; g.max_ratio = 0.f;
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

inline size_t loss_workspace_bytes(const AtssGeom& g) {
    // forward / finalize: 3 partial arrays; backward: one dscale partial per anchor workgroup (fewer)
    return (size_t)3 * (size_t)g.blk0[AT_SEGS] * sizeof(float);
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
        hipLaunchKernelGGL(atss_assign_kernel, dim3(total_gt), dim3(AT_THREADS), 0, (hipStream_t)stream, g, as, gts, keys);
        BRCNN_LAUNCH_CHECK();
    }
    const long long total = (long long)batch * g.n;
    long long grid = (total + 255) / 256;
    if (grid > 8192) grid = 8192;
    hipLaunchKernelGGL(atss_assign_write_kernel, dim3((int)grid), dim3(256), 0, (hipStream_t)stream, g, as, keys, gt_inds,
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
    if (batch < 0 || num_levels <= 0 || num_levels > BRCNN_MAX_LEVELS || num_classes <= 0 ||
        num_classes > 0x7fffff || !topk_inds || !counts || !a || !r || !layout_ok(layout8_host, num_classes) || !scales ||
        !heights || !widths || !strides || !base_anchors_host || !max_shape || !means4_host || !stds4_host ||
        !(wh_ratio_clip > 0.0) || !boxes || !scores || !labels || !valid || !n_valid)
        return BRCNN_EINVAL;
    AtssDecode lv = {};
    lv.num = num_levels; lv.C = num_classes;
    lv.lay = make_layout(layout8_host);
    long long T = 0, rows = 0;
    for (int l = 0; l < num_levels; l++) {
        if (counts[l] <= 0 || !level_ok(heights[l], widths[l], strides[l]) || !topk_inds[l] ||
            counts[l] > (long long)heights[l] * widths[l])
            return BRCNN_EINVAL;
        lv.inds[l] = topk_inds[l];
        lv.hw[l] = heights[l] * widths[l]; lv.width[l] = widths[l]; lv.stride[l] = strides[l];
        for (int k = 0; k < 4; k++) lv.base[l][k] = base_anchors_host[4 * l + k];
        lv.row0[l] = rows;
        rows += (long long)batch * lv.hw[l];
        lv.col0[l] = (int)T;
        T += counts[l];
        if (T * num_classes > 0x7fffffffLL) return BRCNN_EINVAL;
    }
    for (int l = num_levels; l < BRCNN_MAX_LEVELS; l++) { lv.hw[l] = lv.width[l] = lv.stride[l] = 1; }
    for (int l = num_levels; l <= BRCNN_MAX_LEVELS; l++) lv.col0[l] = (int)T;
    lv.T = (int)T;
    for (int k = 0; k < 4; k++) { lv.mean[k] = means4_host[k]; lv.std[k] = stds4_host[k]; }
    lv.max_ratio = (float)fabs(log(wh_ratio_clip));
    lv.score_thr = score_thr;
    if (batch == 0) return 0;
    BRCNN_HIP_CHECK(hipMemsetAsync(n_valid, 0, sizeof(int32_t) * batch, (hipStream_t)stream));
    const long long total = (long long)batch * T * num_classes;
    long long g = (total + 255) / 256;
    if (g > 4096) g = 4096;
    hipLaunchKernelGGL(atss_decode_levels_kernel, dim3((int)g), dim3(256), 0, (hipStream_t)stream, lv, batch, a, r, scales,
                       max_shape, scale_factor, boxes, scores, labels, valid, n_valid);
    BRCNN_LAUNCH_CHECK();
    return 0;
}

BRCNN_API size_t brcnn_atss_loss_workspace_bytes(int batch, int num_levels, const int* heights, const int* widths,
                                                 int num_classes) {
    AtssGeom g;
    int ones[BRCNN_MAX_LEVELS];
    for (int l = 0; l < BRCNN_MAX_LEVELS; l++) ones[l] = 1;
    if (fill_geom(g, batch, num_levels, heights, widths, ones, nullptr, num_classes, nullptr, nullptr, nullptr)) return 0;
    return loss_workspace_bytes(g);
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
        workspace_bytes < loss_workspace_bytes(g))
        return BRCNN_EINVAL;
    float* partials = (float*)workspace;
    hipLaunchKernelGGL(atss_loss_forward_kernel, dim3(g.blk0[AT_SEGS]), dim3(AT_THREADS), 0, (hipStream_t)stream, g, a, r,
                       scales, gt_inds, gts, gt_labels, partials);
    BRCNN_LAUNCH_CHECK();
    hipLaunchKernelGGL(atss_loss_norm_kernel, dim3(1), dim3(AT_THREADS), 0, (hipStream_t)stream, g, gt_inds, partials, norm2);
    BRCNN_LAUNCH_CHECK();
    return 0;
}

BRCNN_API int brcnn_atss_loss_finalize(const void* workspace, size_t workspace_bytes, const float* norm2, int batch,
                                       int num_levels, const int* heights, const int* widths, int num_classes,
                                       const float* cfg15_host, float* losses, float* coef3, void* stream) {
    AtssGeom g;
    int ones[BRCNN_MAX_LEVELS];
    for (int l = 0; l < BRCNN_MAX_LEVELS; l++) ones[l] = 1;
    if (!cfg15_host) return BRCNN_EINVAL;
    const int st = fill_geom(g, batch, num_levels, heights, widths, ones, nullptr, num_classes, nullptr, nullptr, cfg15_host);
    if (st) return st;
    if (!workspace || !norm2 || !losses || !coef3 || workspace_bytes < loss_workspace_bytes(g)) return BRCNN_EINVAL;
    hipLaunchKernelGGL(atss_loss_finalize_kernel, dim3(1), dim3(AT_THREADS), 0, (hipStream_t)stream, g,
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
    if (!a || !r || !scales || !gt_inds || !grad_losses || !coef3 || !workspace || !da || !dr || !dscale ||
        ((!gts || !gt_labels) && g.gt_off[batch] > 0) || workspace_bytes < loss_workspace_bytes(g))
        return BRCNN_EINVAL;
    long long ga = (g.row0[g.L] * g.lay.sa + 255) / 256;
    if (ga > 8192) ga = 8192;
    hipLaunchKernelGGL(atss_loss_backward_a_kernel, dim3((int)ga), dim3(256), 0, (hipStream_t)stream, g, a, r, gt_inds, gts,
                       gt_labels, grad_losses, coef3, da);
    BRCNN_LAUNCH_CHECK();
    float* dsp = (float*)workspace;
    hipLaunchKernelGGL(atss_loss_backward_r_kernel, dim3(g.pblk0[g.L]), dim3(AT_THREADS), 0, (hipStream_t)stream, g, a, r,
                       scales, gt_inds, gts, grad_losses, coef3, dr, dsp);
    BRCNN_LAUNCH_CHECK();
    hipLaunchKernelGGL(atss_dscale_kernel, dim3(1), dim3(AT_THREADS), 0, (hipStream_t)stream, g, dsp, dscale);
    BRCNN_LAUNCH_CHECK();
    return 0;
}
