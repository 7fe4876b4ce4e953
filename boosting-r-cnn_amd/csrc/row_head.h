// What the dense heads on row tensors share (fcos_head.hip, atss_head.hip, gfl_head.hip, vfnet_head.hip): the row layout of
// the head outputs, the pyramid geometry with its split into workgroups, the test-time decode kernel, the block-partial loss
// forward kernel and the dA backward kernel, as templates over a per-head traits type T resolved at compile time.  A head is
// its traits, its assignment, its dR / dD backward, its norm and finalize kernels and its entry points.
//
// What a traits type provides:
//     T::Geom        : RowGeom + what the head's targets need (eps values; base anchors, means / stds; reg_max ...)
//     T::Decode      : RowDecode + what the head's box decode needs; a further row tensor rides in it as a device pointer
//     T::Rows        : the device pointers the loss kernels read, `a` (the class logits) among them
//     T::Cell        : what locate() finds for one row: `gi` (index into the packed gts, < 0 none), + the targets
//     T::PARTIALS    : partial arrays of the forward pass (<= ROW_MAX_PARTIALS)
//     T::HAS_INVALID : gi == -2 marks a row without weight (skipped by the class term)
//     T::HAS_CENTERNESS : the score is class sigmoid * centerness sigmoid, and dA has a centerness column (Cell::ctr_t)
//     T::HAS_QUALITY : the class element of a hit takes a quality q (else q = 0 and quality() is never called)
//     T::decode_box(lv, l, cell, row, raw, scale) -> the box of a picked row before the clip
//     T::locate(g, gt_inds, gts, l, r, want_targets) -> Cell of row r of level l
//     T::quality(g, in, gt_inds, gts, l, r, row) -> q, evaluated by the one thread that has a hit
//     T::cls_elem<BWD>(g, x, hit, q) : the class loss of one (row, class) element, with BWD its derivative w.r.t. x
//     T::point_terms(g, in, o, l, row, acc) : adds the terms of one positive row into acc[0 .. PARTIALS)
//     T::grad(g, term, l) : where the upstream gradient of (term, level l) sits -- g3[term] or gl[term * L + l]
// CenternessTraits<T> below fills in the last six hooks' common part for the heads with a centerness branch, from
//     T::box_term<BWD>(g, cell, raw, scale, dscaled)
// The arithmetic of every expression is the heads' own, operation for operation: the results do not depend on which head
// instantiates a kernel.
#pragma once
#include "decode_tail.h"
#include "head_loss.h"

namespace {

constexpr int CH_THREADS = 256;
constexpr int CH_PER_THREAD = 8;
constexpr int CH_CHUNK = CH_THREADS * CH_PER_THREAD;        // elements (class term) or rows (point terms) per workgroup
constexpr int CH_SEGS = 2 * BRCNN_MAX_LEVELS;               // (level, term): 2 * l = class term, 2 * l + 1 = point terms
constexpr int ROW_MAX_PARTIALS = 5;

// layout8_host (include/brcnn_hip.h); norm_on_bbox and giou are FCOS's switches.  layout4_host fills the first four
struct RowLayout {
    int sa, cls_off, sr, reg_off, ctr_in_r, ctr_off, norm_on_bbox, giou;
};

struct RowGeom {
    int L, C, B, n;                         // n: points (anchors) per image
    int h[BRCNN_MAX_LEVELS], w[BRCNN_MAX_LEVELS], stride[BRCNN_MAX_LEVELS];
    int start[BRCNN_MAX_LEVELS + 1];        // first point of each level within an image
    long long row0[BRCNN_MAX_LEVELS + 1];   // first row of each level in A / R
    int blk0[CH_SEGS + 1];                  // first workgroup of each (level, term) pair
    int pblk0[BRCNN_MAX_LEVELS + 1];        // first workgroup of each level in the backward pass over the rows
    int gt_off[BRCNN_MAX_IMAGES + 1];
    RowLayout lay;
    float gamma, alpha, lw_cls, lw_bbox, lw_ctr;
};

// T::Rows of the heads whose loss reads A, R and the per-level scales
struct ScaledRows {
    const float* __restrict__ a;
    const float* __restrict__ r;
    const float* __restrict__ scales;
};

__device__ __forceinline__ const float* ctr_ptr(const RowLayout& y, const float* a, const float* r, size_t row) {
    return y.ctr_in_r ? r + row * y.sr + y.ctr_off : a + row * y.sa + y.ctr_off;
}

__device__ __forceinline__ int level_of_row(const RowGeom& g, long long row) {
    int l = 0;
#pragma unroll
    for (int i = 1; i < BRCNN_MAX_LEVELS; i++)
        if (i < g.L && row >= g.row0[i]) l = i;
    return l;
}

__device__ __forceinline__ float block_sum(float v, float* red, int tid) {
    __syncthreads();
    red[tid] = v;
    __syncthreads();
    for (int d = CH_THREADS / 2; d > 0; d >>= 1) {
        if (tid < d) red[tid] += red[tid + d];
        __syncthreads();
    }
    return red[0];
}

// the one anchor of cell `cell` of a level: base + (x * stride, y * stride, x * stride, y * stride), exact in fp32
__device__ __forceinline__ float4 anchor_of(const float* base, int width, int stride, int cell) {
    const float sx = (float)((cell % width) * stride), sy = (float)((cell / width) * stride);
    return make_float4(base[0] + sx, base[1] + sy, base[2] + sx, base[3] + sy);
}

// the sum of partials[which] over the workgroups of (level l, term)
__device__ __forceinline__ float level_sum(const RowGeom& g, const float* __restrict__ partials, int which, int l, int term,
                                           float* red, int tid) {
    const int nblk = g.blk0[CH_SEGS], seg = 2 * l + term;
    float s = 0.f;
    for (int i = g.blk0[seg] + tid; i < g.blk0[seg + 1]; i += CH_THREADS) s += partials[which * nblk + i];
    return block_sum(s, red, tid);
}

// the sum of partials[which] over the workgroups of term `term` (0 class, 1 points) of every level, level by level
__device__ __forceinline__ float term_sum(const RowGeom& g, const float* __restrict__ partials, int which, int term, float* red,
                                          int tid) {
    float total = 0.f;
    for (int l = 0; l < g.L; l++) total += level_sum(g, partials, which, l, term, red, tid);
    return total;
}

// ------------------------------------------------------------------------------------------------------------ test time
struct RowDecode {
    int num, C, T;
    const int64_t* inds[BRCNN_MAX_LEVELS];
    int hw[BRCNN_MAX_LEVELS], width[BRCNN_MAX_LEVELS], stride[BRCNN_MAX_LEVELS], col0[BRCNN_MAX_LEVELS + 1];
    long long row0[BRCNN_MAX_LEVELS];
    RowLayout lay;
    float score_thr;
};

// everything between the top-k and multiclass_nms, one thread per (image, pick, class): valid = class sigmoid > score_thr
// -- the class score alone, multiclass_nms masks before it applies a score factor --, score = class sigmoid (* centerness
// sigmoid with T::HAS_CENTERNESS), (level, pick, class) slot order
template <class T>
__global__ __launch_bounds__(256) void rows_decode_levels_kernel(const typename T::Decode lv, int batch,
                                                                const float* __restrict__ a, const float* __restrict__ r,
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
        cell = cell < 0 ? 0 : (cell >= lv.hw[l] ? lv.hw[l] - 1 : cell);     // (a picked index is a cell of the level)
        const size_t row = (size_t)(lv.row0[l] + (long long)b * lv.hw[l] + cell);
        const float s = sigmoidf_(a[row * lv.lay.sa + lv.lay.cls_off + c]);
        float score = s;
        if constexpr (T::HAS_CENTERNESS) score = s * sigmoidf_(*ctr_ptr(lv.lay, a, r, row));
        const float4 o = T::decode_box(lv, l, (int)cell, row, r + row * lv.lay.sr + lv.lay.reg_off, scales[l]);
        store_candidate(t, b, c, o.x, o.y, o.z, o.w, score, s > lv.score_thr, max_shape, scale_factor, boxes, scores, labels,
                        valid, n_valid);
    }
}

// ----------------------------------------------------------------------------------------------------------------- loss
// partials: T::PARTIALS arrays of `nblk` floats.  A class workgroup writes [sum, 0, ...]; a point workgroup what
// T::point_terms adds up
template <class T>
__global__ __launch_bounds__(256) void rows_loss_forward_kernel(const typename T::Geom g, const typename T::Rows in,
                                                               const int* __restrict__ gt_inds,
                                                               const float* __restrict__ gts,
                                                               const int64_t* __restrict__ gt_labels,
                                                               float* __restrict__ partials) {
    static_assert(T::PARTIALS <= ROW_MAX_PARTIALS, "acc[] holds ROW_MAX_PARTIALS sums");
    __shared__ float red[CH_THREADS];
    const int blk = blockIdx.x, tid = threadIdx.x, nblk = g.blk0[CH_SEGS];
    int seg = 0;
#pragma unroll
    for (int i = 1; i < CH_SEGS; i++)
        if (i < 2 * g.L && blk >= g.blk0[i]) seg = i;
    const int l = seg >> 1;
    const bool points = seg & 1;
    const long long rows = (long long)g.B * g.h[l] * g.w[l];
    const long long total = points ? rows : rows * g.C;
    const long long e0 = (long long)(blk - g.blk0[seg]) * CH_CHUNK;
    float acc[ROW_MAX_PARTIALS] = {0.f, 0.f, 0.f, 0.f, 0.f};
    for (int j = 0; j < CH_PER_THREAD; j++) {
        const long long e = e0 + (long long)j * CH_THREADS + tid;
        if (e >= total) break;
        if (!points) {
            const long long rr = e / g.C;
            const int c = (int)(e - rr * g.C);
            const typename T::Cell o = T::locate(g, gt_inds, gts, l, rr, false);
            if (T::HAS_INVALID && o.gi == -2) continue;
            const size_t row = (size_t)(g.row0[l] + rr);
            const bool hit = o.gi >= 0 && gt_labels[o.gi] == c;
            float q = 0.f;
            if constexpr (T::HAS_QUALITY) {
                if (hit) q = T::quality(g, in, gt_inds, gts, l, rr, row);
            }
            acc[0] += T::template cls_elem<false>(g, in.a[row * g.lay.sa + g.lay.cls_off + c], hit, q);
        } else {
            const typename T::Cell o = T::locate(g, gt_inds, gts, l, e, true);
            if (o.gi < 0) continue;
            T::point_terms(g, in, o, l, (size_t)(g.row0[l] + e), acc);
        }
    }
#pragma unroll
    for (int k = 0; k < T::PARTIALS; k++) {
        const float s = block_sum(acc[k], red, tid);
        if (tid == 0) partials[k * nblk + blk] = s;
    }
}

// one thread per element of dA (rows, stride_a), padding columns included: every element is written.  The centerness column
// test is compiled in only with T::HAS_CENTERNESS: under a zero-filled layout4 it would match channel 0
template <class T>
__global__ __launch_bounds__(256) void rows_loss_backward_a_kernel(const typename T::Geom g, const typename T::Rows in,
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
        const bool is_ctr = T::HAS_CENTERNESS && !g.lay.ctr_in_r && ch == g.lay.ctr_off;
        float v = 0.f;
        if (is_cls || is_ctr) {
            const int l = level_of_row(g, row);
            const typename T::Cell o = T::locate(g, gt_inds, gts, l, row - g.row0[l], is_ctr);
            if (is_cls) {
                if (!T::HAS_INVALID || o.gi != -2) {
                    const bool hit = o.gi >= 0 && gt_labels[o.gi] == ch - g.lay.cls_off;
                    float q = 0.f;
                    if constexpr (T::HAS_QUALITY) {
                        if (hit) q = T::quality(g, in, gt_inds, gts, l, row - g.row0[l], (size_t)row);
                    }
                    v = gl[T::grad(g, 0, l)] * coef3[0] * T::template cls_elem<true>(g, in.a[e], hit, q);
                }
            } else if constexpr (T::HAS_CENTERNESS) {
                if (o.gi >= 0) v = gl[T::grad(g, 2, l)] * coef3[2] * (sigmoidf_(in.a[e]) - o.ctr_t);
            }
        }
        da[e] = v;
    }
}

template <class T>
__global__ __launch_bounds__(256) void rows_dscale_kernel(const typename T::Geom g, const float* __restrict__ dscale_partials,
                                                         float* __restrict__ dscale) {
    __shared__ float red[CH_THREADS];
    const int tid = threadIdx.x;
    for (int l = 0; l < g.L; l++) {
        float s = 0.f;
        for (int i = g.pblk0[l] + tid; i < g.pblk0[l + 1]; i += CH_THREADS) s += dscale_partials[i];
        const float t = block_sum(s, red, tid);
        if (tid == 0) dscale[l] = t;
    }
}

// The normalisers of the anchor heads whose gt_inds follow brcnn_atss_assign (atss_head.hip, gfl_head.hip): norm2 = [sum over
// images of max(number of positives, 1), sum of partials[2] over the point workgroups (ATSS: the centerness targets; GFL:
// the positives' weights)]; a count is an integer below 2^24, exact in fp32
template <class T>
__global__ __launch_bounds__(256) void anchor_loss_norm_kernel(const typename T::Geom g, const int* __restrict__ gt_inds,
                                                              const float* __restrict__ partials, float* __restrict__ norm2) {
    __shared__ float red[CH_THREADS];
    const int tid = threadIdx.x;
    float cnt = 0.f;
    for (int b = 0; b < g.B; b++) {
        const int G = g.gt_off[b + 1] - g.gt_off[b];
        float c = 0.f;
        for (int i = tid; i < g.n; i += CH_THREADS) {
            const int gi = gt_inds[(size_t)b * g.n + i];
            c += (gi > 0 && gi <= G) ? 1.f : 0.f;
        }
        cnt += fmaxf(block_sum(c, red, tid), 1.f);
    }
    const float sum = term_sum(g, partials, 2, 1, red, tid);
    if (tid == 0) { norm2[0] = cnt; norm2[1] = sum; }
}

// ------------------------------------------------------------------------------------- the heads with a centerness branch
// The hooks FCOS and ATSS share, over the head's own Geom / Decode / Cell / locate / decode_box / box_term / grad: sigmoid
// focal loss, no quality, and the point terms [box loss * centerness target, centerness BCE, centerness target, 1]
template <class T>
struct CenternessTraits {
    using Rows = ScaledRows;
    static constexpr bool HAS_CENTERNESS = true;
    static constexpr bool HAS_QUALITY = false;

    template <bool BWD, class Geom>
    static __device__ __forceinline__ float cls_elem(const Geom& g, float x, bool hit, float) {
        return focal_elem<BWD>(x, hit, g.gamma, g.alpha);
    }

    template <class Geom, class Cell>
    static __device__ __forceinline__ void point_terms(const Geom& g, const ScaledRows& in, const Cell& o, int l, size_t row,
                                                       float* acc) {
        acc[0] += T::template box_term<false>(g, o, in.r + row * g.lay.sr + g.lay.reg_off, in.scales[l], nullptr) * o.ctr_t;
        acc[1] += bce_logits(*ctr_ptr(g.lay, in.a, in.r, row), o.ctr_t);
        acc[2] += o.ctr_t;
        acc[3] += 1.f;
    }
};

// one thread per row of dR (rows, stride_r): the 4 box columns, the centerness column when it rides on R, zeros elsewhere;
// and per workgroup the partial of dscale_l = sum over the level's rows of d(scaled) * raw
template <class T>
__global__ __launch_bounds__(256) void centerness_loss_backward_r_kernel(const typename T::Geom g, const float* __restrict__ a,
                                                                        const float* __restrict__ r,
                                                                        const float* __restrict__ scales,
                                                                        const int* __restrict__ gt_inds,
                                                                        const float* __restrict__ gts,
                                                                        const float* __restrict__ gl,
                                                                        const float* __restrict__ coef3,
                                                                        float* __restrict__ dr,
                                                                        float* __restrict__ dscale_partials) {
    __shared__ float red[CH_THREADS];
    const int blk = blockIdx.x, tid = threadIdx.x;
    int l = 0;
#pragma unroll
    for (int i = 1; i < BRCNN_MAX_LEVELS; i++)
        if (i < g.L && blk >= g.pblk0[i]) l = i;
    const long long rows = (long long)g.B * g.h[l] * g.w[l];
    const long long e0 = (long long)(blk - g.pblk0[l]) * CH_CHUNK;
    float acc = 0.f;
    for (int j = 0; j < CH_PER_THREAD; j++) {
        const long long e = e0 + (long long)j * CH_THREADS + tid;
        if (e >= rows) break;
        const size_t row = (size_t)(g.row0[l] + e);
        float* out = dr + row * g.lay.sr;
        const typename T::Cell o = T::locate(g, gt_inds, gts, l, e, true);
        float ds[4] = {0.f, 0.f, 0.f, 0.f}, dc = 0.f;
        if (o.gi >= 0) {
            const float* raw = r + row * g.lay.sr + g.lay.reg_off;
            const float sc = scales[l];
            T::template box_term<true>(g, o, raw, sc, ds);
            const float k = gl[T::grad(g, 1, l)] * coef3[1] * o.ctr_t;
#pragma unroll
            for (int q = 0; q < 4; q++) {
                ds[q] = k * ds[q];
                acc += ds[q] * raw[q];
                ds[q] = ds[q] * sc;
            }
            if (g.lay.ctr_in_r)
                dc = gl[T::grad(g, 2, l)] * coef3[2] * (sigmoidf_(r[row * g.lay.sr + g.lay.ctr_off]) - o.ctr_t);
        }
        for (int ch = 0; ch < g.lay.sr; ch++) {
            const int q = ch - g.lay.reg_off;
            out[ch] = (q >= 0 && q < 4) ? ds[q] : ((g.lay.ctr_in_r && ch == g.lay.ctr_off) ? dc : 0.f);
        }
    }
    const float s = block_sum(acc, red, tid);
    if (tid == 0) dscale_partials[blk] = s;
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

RowLayout make_layout(const int* v) {
    RowLayout y;
    y.sa = v[0]; y.cls_off = v[1]; y.sr = v[2]; y.reg_off = v[3]; y.ctr_in_r = v[4] != 0; y.ctr_off = v[5];
    y.norm_on_bbox = v[6] != 0; y.giou = v[7] != 0;
    return y;
}

// layout4_host = [stride_a, cls_off, stride_r, reg_off] of a head without a centerness; its box columns are box_width wide
bool layout4_ok(const int* v, int C, int box_width) {
    return v && v[0] > 0 && v[2] > 0 && v[1] >= 0 && v[3] >= 0 && v[1] + C <= v[0] && v[3] + box_width <= v[2];
}

RowLayout make_layout4(const int* v) {
    RowLayout y = {};
    y.sa = v[0]; y.cls_off = v[1]; y.sr = v[2]; y.reg_off = v[3];
    return y;
}

bool level_ok(int h, int w, int stride) {
    return h > 0 && w > 0 && stride > 0 && stride <= 0x7fff && (long long)h * w <= 0x7fffffffLL &&
           (long long)h * stride <= 0x7fffffLL && (long long)w * stride <= 0x7fffffLL;
}

// the strides of an entry that needs only the pyramid's split into workgroups
struct UnitStrides {
    int v[BRCNN_MAX_LEVELS];
    UnitStrides() { for (int l = 0; l < BRCNN_MAX_LEVELS; l++) v[l] = 1; }
};

// the grid of a grid-stride kernel over n elements or rows
int rows_grid(long long n) {
    long long grid = (n + 255) / 256;
    return (int)(grid > 8192 ? 8192 : (grid < 1 ? 1 : grid));
}

// the pyramid, its split into workgroups, the ground-truth offsets and the layout; the head's own fill_geom adds its settings
int fill_geom_common(RowGeom& g, int batch, int num_levels, const int* heights, const int* widths, const int* strides, int C,
                     const int* gt_offsets_host, const int* layout8) {
    if (batch <= 0 || batch > BRCNN_MAX_IMAGES || num_levels <= 0 || num_levels > BRCNN_MAX_LEVELS || C <= 0 ||
        C > 0x7fffff || !heights || !widths || !strides)
        return BRCNN_EINVAL;
    g.L = num_levels; g.C = C; g.B = batch;
    long long points = 0, rows = 0, blocks = 0, pblocks = 0;
    for (int l = 0; l < num_levels; l++) {
        if (!level_ok(heights[l], widths[l], strides[l])) return BRCNN_EINVAL;
        g.h[l] = heights[l]; g.w[l] = widths[l]; g.stride[l] = strides[l];
        g.start[l] = (int)points;
        g.row0[l] = rows;
        const long long cells = (long long)batch * heights[l] * widths[l];
        points += (long long)heights[l] * widths[l];
        rows += cells;
        g.blk0[2 * l] = (int)blocks;
        blocks += (cells * C + CH_CHUNK - 1) / CH_CHUNK;
        g.blk0[2 * l + 1] = (int)blocks;
        blocks += (cells + CH_CHUNK - 1) / CH_CHUNK;
        g.pblk0[l] = (int)pblocks;
        pblocks += (cells + CH_CHUNK - 1) / CH_CHUNK;
        if (points > 0x7fffffffLL / batch || blocks > 0x3fffffffLL) return BRCNN_EINVAL;
    }
    for (int l = num_levels; l < BRCNN_MAX_LEVELS; l++) { g.h[l] = g.w[l] = g.stride[l] = 1; }
    for (int l = num_levels; l <= BRCNN_MAX_LEVELS; l++) { g.start[l] = (int)points; g.row0[l] = rows; g.pblk0[l] = (int)pblocks; }
    for (int s = 2 * num_levels; s <= CH_SEGS; s++) g.blk0[s] = (int)blocks;
    g.n = (int)points;
    for (int b = 0; b <= BRCNN_MAX_IMAGES; b++) g.gt_off[b] = 0;
    if (gt_offsets_host) {
        for (int b = 0; b <= batch; b++) {
            if (gt_offsets_host[b] < 0 || (b > 0 && gt_offsets_host[b] < gt_offsets_host[b - 1])) return BRCNN_EINVAL;
            g.gt_off[b] = gt_offsets_host[b];
        }
        for (int b = batch + 1; b <= BRCNN_MAX_IMAGES; b++) g.gt_off[b] = gt_offsets_host[batch];
    }
    g.lay = RowLayout{};
    if (layout8) {
        if (!layout_ok(layout8, C)) return BRCNN_EINVAL;
        g.lay = make_layout(layout8);
    }
    g.gamma = g.alpha = 0.f; g.lw_cls = g.lw_bbox = g.lw_ctr = 1.f;
    return 0;
}

// forward / finalize: T::PARTIALS partial arrays; backward: one dscale partial per point workgroup (fewer)
template <class T>
inline size_t loss_workspace_bytes(const RowGeom& g) {
    return (size_t)T::PARTIALS * (size_t)g.blk0[CH_SEGS] * sizeof(float);
}

// the picks and the level geometry of `lv`, whatever the layout of the rows (the caller checks and sets lv.lay)
int fill_decode_picks(RowDecode& lv, const int64_t* const* topk_inds, const int* counts, int batch, int num_levels,
                      const int* heights, const int* widths, const int* strides, int num_classes, float score_thr) {
    if (batch < 0 || num_levels <= 0 || num_levels > BRCNN_MAX_LEVELS || num_classes <= 0 || num_classes > 0x7fffff ||
        !topk_inds || !counts || !heights || !widths || !strides)
        return BRCNN_EINVAL;
    lv.num = num_levels; lv.C = num_classes;
    long long T = 0, rows = 0;
    for (int l = 0; l < num_levels; l++) {
        if (counts[l] <= 0 || !level_ok(heights[l], widths[l], strides[l]) || !topk_inds[l] ||
            counts[l] > (long long)heights[l] * widths[l])
            return BRCNN_EINVAL;
        lv.inds[l] = topk_inds[l];
        lv.hw[l] = heights[l] * widths[l]; lv.width[l] = widths[l]; lv.stride[l] = strides[l];
        lv.row0[l] = rows;
        rows += (long long)batch * lv.hw[l];
        lv.col0[l] = (int)T;
        T += counts[l];
        if (T * num_classes > 0x7fffffffLL) return BRCNN_EINVAL;
    }
    for (int l = num_levels; l < BRCNN_MAX_LEVELS; l++) { lv.hw[l] = lv.width[l] = lv.stride[l] = 1; }
    for (int l = num_levels; l <= BRCNN_MAX_LEVELS; l++) lv.col0[l] = (int)T;
    lv.T = (int)T;
    lv.score_thr = score_thr;
    return 0;
}

// the common part of a *_decode_levels entry of the centerness heads: argument checks, layout8, the picks and the geometry
int fill_decode_common(RowDecode& lv, const int64_t* const* topk_inds, const int* counts, const float* a, const float* r,
                       const int* layout8_host, const float* scales, int batch, int num_levels, const int* heights,
                       const int* widths, const int* strides, int num_classes, const float* max_shape, float score_thr,
                       const float* boxes, const float* scores, const int64_t* labels, const uint8_t* valid,
                       const int32_t* n_valid) {
    if (batch < 0 || num_levels <= 0 || num_levels > BRCNN_MAX_LEVELS || num_classes <= 0 ||
        num_classes > 0x7fffff || !topk_inds || !counts || !a || !r || !layout_ok(layout8_host, num_classes) || !scales ||
        !heights || !widths || !strides || !max_shape || !boxes || !scores || !labels || !valid || !n_valid)
        return BRCNN_EINVAL;
    lv.lay = make_layout(layout8_host);
    return fill_decode_picks(lv, topk_inds, counts, batch, num_levels, heights, widths, strides, num_classes, score_thr);
}

// the per-level base anchors of an anchor head's decode
template <class D>
void fill_decode_base(D& lv, const float* base_anchors_host, int num_levels) {
    for (int l = 0; l < num_levels; l++)
        for (int k = 0; k < 4; k++) lv.base[l][k] = base_anchors_host[4 * l + k];
}

template <class T>
int launch_decode_levels(const typename T::Decode& lv, int batch, const float* a, const float* r, const float* scales,
                         const float* max_shape, const float* scale_factor, float* boxes, float* scores, int64_t* labels,
                         uint8_t* valid, int32_t* n_valid, void* stream) {
    if (batch == 0) return 0;
    BRCNN_HIP_CHECK(hipMemsetAsync(n_valid, 0, sizeof(int32_t) * batch, (hipStream_t)stream));
    const long long total = (long long)batch * lv.T * lv.C;
    long long g = (total + 255) / 256;
    if (g > 4096) g = 4096;
    hipLaunchKernelGGL(rows_decode_levels_kernel<T>, dim3((int)g), dim3(256), 0, (hipStream_t)stream, lv, batch, a, r, scales,
                       max_shape, scale_factor, boxes, scores, labels, valid, n_valid);
    BRCNN_LAUNCH_CHECK();
    return 0;
}

// the forward launch of a *_loss_forward entry, after its fill_geom and argument checks; the head's norm kernel follows
template <class T>
int launch_loss_forward(const typename T::Geom& g, const typename T::Rows& in, const int32_t* gt_inds, const float* gts,
                        const int64_t* gt_labels, float* partials, void* stream) {
    hipLaunchKernelGGL(rows_loss_forward_kernel<T>, dim3(g.blk0[CH_SEGS]), dim3(CH_THREADS), 0, (hipStream_t)stream, g, in,
                       gt_inds, gts, gt_labels, partials);
    BRCNN_LAUNCH_CHECK();
    return 0;
}

// the dA launch of a *_loss_backward entry
template <class T>
int launch_loss_backward_a(const typename T::Geom& g, const typename T::Rows& in, const int32_t* gt_inds, const float* gts,
                           const int64_t* gt_labels, const float* grad_losses, const float* coef3, float* da, void* stream) {
    hipLaunchKernelGGL(rows_loss_backward_a_kernel<T>, dim3(rows_grid(g.row0[g.L] * g.lay.sa)), dim3(256), 0,
                       (hipStream_t)stream, g, in, gt_inds, gts, gt_labels, grad_losses, coef3, da);
    BRCNN_LAUNCH_CHECK();
    return 0;
}

// what a *_loss_backward entry on (A, R, scales) checks after its fill_geom
template <class T>
bool loss_backward_args_ok(const typename T::Geom& g, const float* a, const float* r, const float* scales,
                           const int32_t* gt_inds, const float* gts, const int64_t* gt_labels, const float* grad_losses,
                           const float* coef3, const void* workspace, size_t workspace_bytes, const float* da, const float* dr,
                           const float* dscale) {
    return a && r && scales && gt_inds && grad_losses && coef3 && workspace && da && dr && dscale &&
           !((!gts || !gt_labels) && g.gt_off[g.B] > 0) && workspace_bytes >= loss_workspace_bytes<T>(g);
}

// the three launches of a centerness head's *_loss_backward entry, after its fill_geom
template <class T>
int launch_loss_backward(const typename T::Geom& g, const float* a, const float* r, const float* scales,
                         const int32_t* gt_inds, const float* gts, const int64_t* gt_labels, const float* grad_losses,
                         const float* coef3, void* workspace, size_t workspace_bytes, float* da, float* dr, float* dscale,
                         void* stream) {
    if (!loss_backward_args_ok<T>(g, a, r, scales, gt_inds, gts, gt_labels, grad_losses, coef3, workspace, workspace_bytes, da,
                                  dr, dscale))
        return BRCNN_EINVAL;
    const int st = launch_loss_backward_a<T>(g, ScaledRows{a, r, scales}, gt_inds, gts, gt_labels, grad_losses, coef3, da, stream);
    if (st) return st;
    float* dsp = (float*)workspace;
    hipLaunchKernelGGL(centerness_loss_backward_r_kernel<T>, dim3(g.pblk0[g.L]), dim3(CH_THREADS), 0, (hipStream_t)stream, g,
                       a, r, scales, gt_inds, gts, grad_losses, coef3, dr, dsp);
    BRCNN_LAUNCH_CHECK();
    hipLaunchKernelGGL(rows_dscale_kernel<T>, dim3(1), dim3(CH_THREADS), 0, (hipStream_t)stream, g, dsp, dscale);
    BRCNN_LAUNCH_CHECK();
    return 0;
}

}  // namespace
