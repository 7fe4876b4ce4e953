// Test-time augmentation (multi-scale + flip) on the device-resident path: the three small kernels that keep
// TwoStageDetector.aug_test (mmdet/models/detectors/two_stage.py:184-193) free of host round trips.
//
//   tta_gather_proposals: merge_aug_proposals up to its NMS call (core/post_processing/merge_augs.py:61-72): the
//                         proposals of every aug mapped back to the original image (bbox_mapping_back,
//                         core/bbox/transforms.py:47-56) and concatenated aug-major into the candidate slots
//   tta_map_rois        : bbox_mapping (transforms.py:35-44) of the merged proposals into every aug's frame, as RoIs
//   rcnn_decode_tta     : aug_test_bboxes + merge_aug_bboxes (roi_heads/test_mixins.py:138-165, merge_augs.py:84-110):
//                         per (proposal, class) the mean over the augs of the mapped-back decoded box and of the score
//
// Per-(aug, image) geometry is one device table geom (A, B, 8) = [img_h, img_w, sf0, sf1, sf2, sf3, flip, 0]
// (scale_factor as the meta carries it: [sx, sy, sx, sy]; flip 0 none, 1 horizontal, 2 vertical, 3 diagonal).
// Every coordinate is computed with the reference's fp32 operations in its order (`w - x2`, then a true division by
// the scale factor; the library is built without FMA contraction and with correctly rounded division), so the mapped
// boxes equal torch's bit for bit.
#include "common.h"

namespace {

struct Geom {
    float h, w, sf[4];
    int flip;
};

__device__ __forceinline__ Geom load_geom(const float* __restrict__ geom, int a, int b, int B) {
    const float4* g = reinterpret_cast<const float4*>(geom + ((size_t)a * B + b) * 8);
    const float4 lo = g[0], hi = g[1];
    Geom o;
    o.h = lo.x; o.w = lo.y; o.sf[0] = lo.z; o.sf[1] = lo.w; o.sf[2] = hi.x; o.sf[3] = hi.y;
    o.flip = (int)hi.z;
    return o;
}

// bbox_flip (transforms.py:6-32): its own inverse
__device__ __forceinline__ float4 flip_box(float4 v, const Geom& g) {
    float4 o = v;
    if (g.flip & 1) { o.x = g.w - v.z; o.z = g.w - v.x; }
    if (g.flip & 2) { o.y = g.h - v.w; o.w = g.h - v.y; }
    return o;
}

// bbox_mapping_back: un-flip about img_shape, then divide by the scale factor
__device__ __forceinline__ float4 map_back(float4 v, const Geom& g) {
    const float4 f = flip_box(v, g);
    return make_float4(f.x / g.sf[0], f.y / g.sf[1], f.z / g.sf[2], f.w / g.sf[3]);
}

// bbox_mapping: multiply by the scale factor, then flip
__device__ __forceinline__ float4 map_into(float4 v, const Geom& g) {
    return flip_box(make_float4(v.x * g.sf[0], v.y * g.sf[1], v.z * g.sf[2], v.w * g.sf[3]), g);
}

struct AugProposals {
    const float* props[BRCNN_TTA_MAX_AUGS];      // (B, K_a, 5)
    const int* num[BRCNN_TTA_MAX_AUGS];          // (B,)
    int col0[BRCNN_TTA_MAX_AUGS + 1];            // aug a owns columns [col0[a], col0[a+1]) of the T candidate slots
    int A;
};

__global__ __launch_bounds__(256) void tta_gather_kernel(AugProposals ap, const float* __restrict__ geom, int B,
                                                        float* __restrict__ cand, float* __restrict__ boxes,
                                                        float* __restrict__ scores, uint8_t* __restrict__ valid) {
    const int T = ap.col0[ap.A];
    const long long total = (long long)B * T;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total;
         t += (long long)gridDim.x * blockDim.x) {
        const int b = (int)(t / T), col = (int)(t - (long long)b * T);
        int a = 0;
#pragma unroll
        for (int i = 1; i < BRCNN_TTA_MAX_AUGS; i++)
            if (i < ap.A && col >= ap.col0[i]) a = i;
        const int Ka = ap.col0[a + 1] - ap.col0[a], k = col - ap.col0[a];
        const float* p = ap.props[a] + ((size_t)b * Ka + k) * 5;
        const bool ok = k < ap.num[a][b];
        float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
        float s = 0.f;
        if (ok) {
            o = map_back(make_float4(p[0], p[1], p[2], p[3]), load_geom(geom, a, b, B));
            s = p[4];
        }
        float* c = cand + t * 5;
        c[0] = o.x; c[1] = o.y; c[2] = o.z; c[3] = o.w; c[4] = s;
        if (boxes) *reinterpret_cast<float4*>(boxes + t * 4) = o;
        if (scores) scores[t] = s;
        valid[t] = ok ? 1 : 0;
    }
}

__global__ __launch_bounds__(256) void tta_map_rois_kernel(const float* __restrict__ merged, const float* __restrict__ geom,
                                                          int A, int B, int K, float* __restrict__ rois) {
    const long long per_aug = (long long)B * K, total = per_aug * A;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total;
         t += (long long)gridDim.x * blockDim.x) {
        const int a = (int)(t / per_aug);
        const long long bk = t - (long long)a * per_aug;
        const int b = (int)(bk / K);
        const float* p = merged + bk * 5;
        const float4 o = map_into(make_float4(p[0], p[1], p[2], p[3]), load_geom(geom, a, b, B));
        float* r = rois + t * 5;
        r[0] = (float)b; r[1] = o.x; r[2] = o.y; r[3] = o.z; r[4] = o.w;
    }
}

// sum_j exp(x[j] - m) of one row of n logits in the association order of a lane-per-element butterfly reduction over
// W = min(pow2ceil(n), 64) lanes (lane l owns x[l], x[l + W], ...; partners l ^ W/2, l ^ W/4, ..., l ^ 1).  This is the
// order of torch's device softmax for rows of up to 1024 elements, which simple_test's scores go through: with one aug
// the scores of the two paths then coincide.  LEVELS = log2(W) levels remain below (r, step).
template <int LEVELS>
__device__ __forceinline__ float exp_sum_tree(const float* __restrict__ x, int n, float m, int r, int step, int W) {
    if constexpr (LEVELS == 0) {
        float s = 0.f;
        for (int j = r; j < n; j += W) s += expf(x[j] - m);
        return s;
    } else {
        return exp_sum_tree<LEVELS - 1>(x, n, m, r, step * 2, W) + exp_sum_tree<LEVELS - 1>(x, n, m, r + step, step * 2, W);
    }
}

__device__ __forceinline__ float exp_sum(const float* __restrict__ x, int n, float m) {
    if (n <= 2) return exp_sum_tree<1>(x, n, m, 0, 1, 2);
    if (n <= 4) return exp_sum_tree<2>(x, n, m, 0, 1, 4);
    if (n <= 8) return exp_sum_tree<3>(x, n, m, 0, 1, 8);
    if (n <= 16) return exp_sum_tree<4>(x, n, m, 0, 1, 16);
    if (n <= 32) return exp_sum_tree<5>(x, n, m, 0, 1, 32);
    return exp_sum_tree<6>(x, n, m, 0, 1, 64);
}

struct TtaDecodeParams {
    float mean[4], std[4];
    float max_ratio, score_thr;
    int raw;        // 0: mean of sqrt(softmax * prior)   1: mean of the logits (the reference's literal behaviour)
};

__global__ __launch_bounds__(256) void rcnn_decode_tta_kernel(
    const float* __restrict__ cls_score, const float* __restrict__ bbox_pred, const float* __restrict__ merged,
    const int* __restrict__ num, const float* __restrict__ geom, const float* __restrict__ out_scale, int A, int B, int K,
    int C, TtaDecodeParams dp, float* __restrict__ boxes, float* __restrict__ scores, int64_t* __restrict__ labels,
    uint8_t* __restrict__ valid) {
    const long long rows = (long long)B * K, total = rows * C;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total;
         t += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(t % C);
        const long long bk = t / C;
        const int b = (int)(bk / K), k = (int)(bk - (long long)b * K);
        const float* pr = merged + bk * 5;           // x1, y1, x2, y2, prior: original frame
        const float4 p0 = make_float4(pr[0], pr[1], pr[2], pr[3]);
        const float prior = pr[4];
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        float sacc = 0.f;
        for (int a = 0; a < A; a++) {
            const Geom g = load_geom(geom, a, b, B);
            const float* row = cls_score + ((size_t)a * rows + bk) * (C + 1);
            float s;
            if (dp.raw) {
                s = row[c];
            } else {
                float m = row[0];
                for (int j = 1; j <= C; j++) m = fmaxf(m, row[j]);
                s = sqrtf(expf(row[c] - m) / exp_sum(row, C + 1, m) * prior);
            }
            sacc = a == 0 ? s : sacc + s;
            // delta2bbox (delta_xywh_bbox_coder.py:145-272) of the proposal in this aug's frame, clipped at its img_shape
            const float4 r = map_into(p0, g);
            const float4 d = *reinterpret_cast<const float4*>(bbox_pred + ((size_t)a * rows + bk) * 4 * C + 4 * c);
            const float dx = d.x * dp.std[0] + dp.mean[0];
            const float dy = d.y * dp.std[1] + dp.mean[1];
            float dw = d.z * dp.std[2] + dp.mean[2];
            float dh = d.w * dp.std[3] + dp.mean[3];
            const float px = (r.x + r.z) * 0.5f, py = (r.y + r.w) * 0.5f;
            const float pw = r.z - r.x, ph = r.w - r.y;
            const float dxw = pw * dx, dyh = ph * dy;
            dw = fminf(fmaxf(dw, -dp.max_ratio), dp.max_ratio);
            dh = fminf(fmaxf(dh, -dp.max_ratio), dp.max_ratio);
            const float gw = pw * expf(dw), gh = ph * expf(dh);
            const float gx = px + dxw, gy = py + dyh;
            float4 o = make_float4(gx - gw * 0.5f, gy - gh * 0.5f, gx + gw * 0.5f, gy + gh * 0.5f);
            o.x = o.x < 0.f ? 0.f : o.x; o.x = o.x > g.w ? g.w : o.x;
            o.y = o.y < 0.f ? 0.f : o.y; o.y = o.y > g.h ? g.h : o.y;
            o.z = o.z < 0.f ? 0.f : o.z; o.z = o.z > g.w ? g.w : o.z;
            o.w = o.w < 0.f ? 0.f : o.w; o.w = o.w > g.h ? g.h : o.w;
            o = map_back(o, g);
            if (a == 0) {
                acc = o;
            } else {
                acc.x += o.x; acc.y += o.y; acc.z += o.z; acc.w += o.w;
            }
        }
        const float fa = (float)A;
        float4 o = make_float4(acc.x / fa, acc.y / fa, acc.z / fa, acc.w / fa);
        const float s = sacc / fa;
        if (out_scale) {
            const float* sf = out_scale + 4 * b;
            o.x *= sf[0]; o.y *= sf[1]; o.z *= sf[2]; o.w *= sf[3];
        }
        *reinterpret_cast<float4*>(boxes + t * 4) = o;
        scores[t] = s;
        labels[t] = c;
        valid[t] = (s > dp.score_thr && k < num[b]) ? 1 : 0;
    }
}

inline int grid_for(long long total) {
    long long g = (total + 255) / 256;
    return (int)(g > 4096 ? 4096 : (g < 1 ? 1 : g));
}

}  // namespace

BRCNN_API int brcnn_tta_gather_proposals(const float* const* proposals, const int32_t* const* num, const int* per_aug_host,
                                         int num_augs, const float* geom, int batch, float* candidates, float* boxes,
                                         float* scores, uint8_t* valid, void* stream) {
    if (!proposals || !num || !per_aug_host || !geom || !candidates || !valid || batch <= 0 || num_augs <= 0 ||
        num_augs > BRCNN_TTA_MAX_AUGS)
        return BRCNN_EINVAL;
    AugProposals ap = {};
    ap.A = num_augs;
    long long T = 0;
    for (int a = 0; a < num_augs; a++) {
        if (!proposals[a] || !num[a] || per_aug_host[a] <= 0) return BRCNN_EINVAL;
        ap.props[a] = proposals[a];
        ap.num[a] = num[a];
        ap.col0[a] = (int)T;
        T += per_aug_host[a];
        if (T > (1 << 24)) return BRCNN_EINVAL;
    }
    ap.col0[num_augs] = (int)T;
    hipLaunchKernelGGL(tta_gather_kernel, dim3(grid_for((long long)batch * T)), dim3(256), 0, (hipStream_t)stream, ap, geom,
                       batch, candidates, boxes, scores, valid);
    BRCNN_LAUNCH_CHECK();
    return 0;
}

BRCNN_API int brcnn_tta_map_rois(const float* merged, const float* geom, int num_augs, int batch, int per_image,
                                 float* rois, void* stream) {
    if (!merged || !geom || !rois || batch <= 0 || per_image <= 0 || num_augs <= 0 || num_augs > BRCNN_TTA_MAX_AUGS)
        return BRCNN_EINVAL;
    hipLaunchKernelGGL(tta_map_rois_kernel, dim3(grid_for((long long)num_augs * batch * per_image)), dim3(256), 0,
                       (hipStream_t)stream, merged, geom, num_augs, batch, per_image, rois);
    BRCNN_LAUNCH_CHECK();
    return 0;
}

BRCNN_API int brcnn_rcnn_decode_tta(const float* cls_score, const float* bbox_pred, const float* merged, const int32_t* num,
                                    const float* geom, const float* out_scale, int num_augs, int batch, int per_image,
                                    int num_classes, int mode, float score_thr, const float* means4_host,
                                    const float* stds4_host, double wh_ratio_clip, float* boxes, float* scores,
                                    int64_t* labels, uint8_t* valid, void* stream) {
    if (!cls_score || !bbox_pred || !merged || !num || !geom || !boxes || !scores || !labels || !valid || batch <= 0 ||
        per_image <= 0 || num_classes <= 0 || num_augs <= 0 || num_augs > BRCNN_TTA_MAX_AUGS ||
        (mode != BRCNN_TTA_FUSED && mode != BRCNN_TTA_RAW) || !means4_host || !stds4_host || !(wh_ratio_clip > 0.0))
        return BRCNN_EINVAL;
    TtaDecodeParams dp = {};
    for (int i = 0; i < 4; i++) { dp.mean[i] = means4_host[i]; dp.std[i] = stds4_host[i]; }
    dp.max_ratio = (float)fabs(log(wh_ratio_clip));
    dp.score_thr = score_thr;
    dp.raw = mode == BRCNN_TTA_RAW;
    hipLaunchKernelGGL(rcnn_decode_tta_kernel, dim3(grid_for((long long)batch * per_image * num_classes)), dim3(256), 0,
                       (hipStream_t)stream, cls_score, bbox_pred, merged, num, geom, out_scale, num_augs, batch, per_image,
                       num_classes, dp, boxes, scores, labels, valid);
    BRCNN_LAUNCH_CHECK();
    return 0;
}
