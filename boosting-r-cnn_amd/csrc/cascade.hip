// Cascade R-CNN: handing boxes from one stage to the next (CascadeRoIHead,
// mmdet/models/roi_heads/cascade_roi_head.py:191-400; BBoxHead.refine_bboxes / regress_by_class,
// roi_heads/bbox_heads/bbox_head.py:382-498).  The reference does this per image with nonzero / gather /
// decode / boolean indexing / cat, three times per step; here each is ONE launch on the padded (B, K, 5)
// layout the sampler and the RoI extractor use, and nothing is read back to the host.
//
//   cascade_refine_test  : between two test-time stages (:342-372).  G = the power of two >= C+1 (at most 64)
//                          lanes share a row: they read its logits side by side (consecutive lanes, consecutive
//                          addresses), add them into logit_sum on the way, reduce (value, index) pairs to the
//                          arg-max of the C foreground columns (lowest index on ties, torch's rule) and lane 0
//                          of the group decodes the label's four deltas, clips and writes the row of dets_out.
//   cascade_mean_softmax : the ensemble of :374-378 + the softmax of BBoxHead.get_bboxes, same row layout:
//                          (logit_sum + last) / num_stages, max, exp, sum, one division per column.
//   cascade_refine_train : refine_bboxes (:264-284 of the RoI head).  One workgroup per image: the wave groups
//                          first find the arg-max label of the image's background rows (class-specific heads
//                          only; an agnostic head's deltas do not depend on the label), then one thread per
//                          row decodes, and the rows that are not added ground truth are compacted in their
//                          original order with wave prefix sums over the keep flags (the compaction of
//                          rpn_sampled_draw), 1024 rows per pass.
//
// Logits and deltas are fp32 in every compute mode (the heads' last GEMM writes fp32).  Plain vector stores,
// no float atomics, no order that depends on scheduling: two runs give the same bits.  delta2bbox
// (core/bbox/coder/delta_xywh_bbox_coder.py:145-272) in the reference's operation order, no FMA contraction.
#include "common.h"
#include <math.h>

namespace {

constexpr int CASCADE_MAX_ROWS = 2048;      // rows of one image the train-time refinement serves: the sampler's limit

struct CascadeCoder {
    float mean[4], std[4];
    float max_ratio;
};

__device__ __forceinline__ float4 cascade_decode(float x1, float y1, float x2, float y2, float d0, float d1, float d2,
                                                 float d3, const CascadeCoder& cd, float mh, float mw) {
    const float dx = d0 * cd.std[0] + cd.mean[0];
    const float dy = d1 * cd.std[1] + cd.mean[1];
    float dw = d2 * cd.std[2] + cd.mean[2];
    float dh = d3 * cd.std[3] + cd.mean[3];
    const float px = (x1 + x2) * 0.5f, py = (y1 + y2) * 0.5f;
    const float pw = x2 - x1, ph = y2 - y1;
    const float dxw = pw * dx, dyh = ph * dy;
    dw = fminf(fmaxf(dw, -cd.max_ratio), cd.max_ratio);
    dh = fminf(fmaxf(dh, -cd.max_ratio), cd.max_ratio);
    const float gw = pw * expf(dw), gh = ph * expf(dh);
    const float gx = px + dxw, gy = py + dyh;
    float ox1 = gx - gw * 0.5f, oy1 = gy - gh * 0.5f;
    float ox2 = gx + gw * 0.5f, oy2 = gy + gh * 0.5f;
    ox1 = ox1 < 0.f ? 0.f : ox1; ox1 = ox1 > mw ? mw : ox1;
    oy1 = oy1 < 0.f ? 0.f : oy1; oy1 = oy1 > mh ? mh : oy1;
    ox2 = ox2 < 0.f ? 0.f : ox2; ox2 = ox2 > mw ? mw : ox2;
    oy2 = oy2 < 0.f ? 0.f : oy2; oy2 = oy2 > mh ? mh : oy2;
    return make_float4(ox1, oy1, ox2, oy2);
}

// (value, index) of the larger logit; the lower index on equal values
__device__ __forceinline__ void argmax_take(float& v, int& i, float ov, int oi) {
    if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
}

// arg-max over columns [0, C) of one row by the G lanes of its group (sub = lane within the group).  Every lane of
// the group returns the same index.  `acc` != NULL: the row's C+1 logits are also accumulated into it on the way.
__device__ __forceinline__ int group_argmax(const float* __restrict__ row, int C, int G, int sub, bool live,
                                            float* __restrict__ acc, bool first) {
    float v = -INFINITY;
    int idx = 0x7fffffff;
    if (live) {
        for (int c = sub; c <= C; c += G) {
            const float x = row[c];
            if (acc) acc[c] = first ? x : acc[c] + x;
            if (c < C) argmax_take(v, idx, x, c);       // (ascending c: a later equal value does not replace)
        }
    }
    for (int d = G >> 1; d > 0; d >>= 1) {
        const float ov = __shfl_xor(v, d, 64);
        const int oi = __shfl_xor(idx, d, 64);
        argmax_take(v, idx, ov, oi);
    }
    return idx < C ? idx : 0;       // (a row of NaNs orders nothing: column 0)
}

__host__ __device__ inline int cascade_group(int C) {
    int G = 1;
    while (G < C + 1 && G < 64) G <<= 1;
    return G;
}

__global__ __launch_bounds__(256) void cascade_refine_test_kernel(
    const float* __restrict__ dets, const int* __restrict__ num, const float* __restrict__ cls, int cls_stride,
    const float* __restrict__ reg, int reg_stride, const float* __restrict__ max_shape, int B, int K, int C, int G,
    int agnostic, int first, CascadeCoder cd, float* __restrict__ dets_out, float* __restrict__ logit_sum) {
    const int sub = threadIdx.x & (G - 1);
    const long long total = (long long)B * K;
    const long long r = ((long long)blockIdx.x * 256 + threadIdx.x) / G;
    const bool live = r < total;
    const long long rr = live ? r : 0;
    const int label = group_argmax(cls + rr * cls_stride, C, G, sub, live, logit_sum + rr * (C + 1), first != 0);
    if (!live || sub != 0) return;
    const int b = (int)(r / K), k = (int)(r - (long long)b * K);
    float* o = dets_out + r * 5;
    float4 bx = make_float4(0.f, 0.f, 0.f, 0.f);
    if (k < num[b]) {
        const float* p = dets + r * 5;
        const float* d = reg + r * reg_stride + (agnostic ? 0 : 4 * label);
        bx = cascade_decode(p[0], p[1], p[2], p[3], d[0], d[1], d[2], d[3], cd, max_shape[2 * b], max_shape[2 * b + 1]);
    }
    o[0] = bx.x; o[1] = bx.y; o[2] = bx.z; o[3] = bx.w; o[4] = 0.f;
}

__global__ __launch_bounds__(256) void cascade_mean_softmax_kernel(const float* __restrict__ logit_sum,
                                                                  const float* __restrict__ cls, int cls_stride,
                                                                  long long rows, int C, int G, float stages,
                                                                  float* __restrict__ probs,
                                                                  float* __restrict__ mean_out) {
    const int sub = threadIdx.x & (G - 1);
    const long long r = ((long long)blockIdx.x * 256 + threadIdx.x) / G;
    const bool live = r < rows;
    const long long rr = live ? r : 0;
    const float* s = logit_sum ? logit_sum + rr * (C + 1) : nullptr;
    const float* x = cls + rr * cls_stride;
    // the mean is formed the same way in every pass (fp32 adds in stage order, one division): same bits each time
    float m = -INFINITY;
    if (live)
        for (int c = sub; c <= C; c += G) m = fmaxf(m, (s ? s[c] + x[c] : x[c]) / stages);
    for (int d = G >> 1; d > 0; d >>= 1) m = fmaxf(m, __shfl_xor(m, d, 64));
    float sum = 0.f;
    if (live)
        for (int c = sub; c <= C; c += G) sum += expf((s ? s[c] + x[c] : x[c]) / stages - m);
    for (int d = G >> 1; d > 0; d >>= 1) sum += __shfl_xor(sum, d, 64);     // (a + b == b + a: every lane the same bits)
    if (live)
        for (int c = sub; c <= C; c += G) {
            const float mean = (s ? s[c] + x[c] : x[c]) / stages;
            probs[rr * (C + 1) + c] = expf(mean - m) / sum;
            if (mean_out) mean_out[rr * (C + 1) + c] = mean;
        }
}

struct RefineTrainParams {
    const float* rois;          // (N, 5) [image, x1, y1, x2, y2]
    const long long* labels;    // (N)
    const int* gt_flags;        // (N) 1 = ground truth added by the sampler
    int row0[BRCNN_MAX_IMAGES + 1];
    const float* cls;           // (N, C+1), row stride cls_stride
    const float* reg;           // (N, 4 | 4C), row stride reg_stride
    int cls_stride, reg_stride;
    const float* max_shape;     // (B, 2)
    int C, G, agnostic, Kout;
    CascadeCoder cd;
    float* props_out;           // (B, Kout, 5)
    int* num_out;               // (B)
};

__global__ __launch_bounds__(1024) void cascade_refine_train_kernel(const RefineTrainParams p) {
    __shared__ int s_label[CASCADE_MAX_ROWS];
    __shared__ int wsum[16];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r0 = p.row0[b], rows = p.row0[b + 1] - r0;
    for (int j = tid; j < rows; j += 1024) s_label[j] = (int)p.labels[r0 + j];
    __syncthreads();
    if (!p.agnostic) {
        // background rows take the arg-max foreground class (cascade_roi_head.py:279-281)
        const int G = p.G, sub = tid & (G - 1), per_pass = 1024 / G;
        for (int j0 = 0; j0 < rows; j0 += per_pass) {
            const int j = j0 + tid / G;
            const bool need = j < rows && s_label[j] == p.C;
            const int am = group_argmax(p.cls + (size_t)(r0 + (need ? j : 0)) * p.cls_stride, p.C, G, sub, need, nullptr,
                                        false);
            if (need && sub == 0) s_label[j] = am;
        }
        __syncthreads();
    }
    const float mh = p.max_shape[2 * b], mw = p.max_shape[2 * b + 1];
    float* out = p.props_out + (size_t)b * p.Kout * 5;
    int base = 0;
    for (int j0 = 0; j0 < rows; j0 += 1024) {
        const int j = j0 + tid;
        const bool keep = j < rows && p.gt_flags[r0 + j] == 0;
        const unsigned long long bal = __ballot(keep);
        if (lane == 0) wsum[wave] = __popcll(bal);
        __syncthreads();
        int off = __popcll(bal & ((1ull << lane) - 1ull)), tot = 0;
        for (int w = 0; w < 16; w++) {
            if (w < wave) off += wsum[w];
            tot += wsum[w];
        }
        if (keep) {
            const size_t r = (size_t)(r0 + j);
            const float* ro = p.rois + r * 5;
            int label = s_label[j];
            label = label < 0 ? 0 : (label >= p.C ? p.C - 1 : label);
            const float* d = p.reg + r * p.reg_stride + (p.agnostic ? 0 : 4 * label);
            const float4 bx = cascade_decode(ro[1], ro[2], ro[3], ro[4], d[0], d[1], d[2], d[3], p.cd, mh, mw);
            float* o = out + (size_t)(base + off) * 5;
            o[0] = bx.x; o[1] = bx.y; o[2] = bx.z; o[3] = bx.w; o[4] = 0.f;
        }
        base += tot;
        __syncthreads();
    }
    for (int i = base * 5 + tid; i < p.Kout * 5; i += 1024) out[i] = 0.f;
    if (tid == 0) p.num_out[b] = base;
}

int fill_coder(CascadeCoder& cd, const float* means4_host, const float* stds4_host, double wh_ratio_clip) {
    if (!means4_host || !stds4_host || !(wh_ratio_clip > 0.0)) return BRCNN_EINVAL;
    for (int i = 0; i < 4; i++) { cd.mean[i] = means4_host[i]; cd.std[i] = stds4_host[i]; }
    cd.max_ratio = (float)fabs(log(wh_ratio_clip));
    return 0;
}

}  // namespace

BRCNN_API int brcnn_cascade_refine_test(const float* dets, const int32_t* num, const float* cls_score, int cls_stride,
                                        const float* bbox_pred, int reg_stride, const float* max_shape, int batch,
                                        int per_image, int num_classes, int reg_class_agnostic, int first,
                                        const float* means4_host, const float* stds4_host, double wh_ratio_clip,
                                        float* dets_out, float* logit_sum, void* stream) {
    if (!dets || !num || !cls_score || !bbox_pred || !max_shape || !dets_out || !logit_sum || batch <= 0 ||
        per_image <= 0 || num_classes < 1 || cls_stride < num_classes + 1 ||
        reg_stride < (reg_class_agnostic ? 4 : 4 * num_classes))
        return BRCNN_EINVAL;
    CascadeCoder cd;
    if (int st = fill_coder(cd, means4_host, stds4_host, wh_ratio_clip)) return st;
    const int G = cascade_group(num_classes);
    const long long threads = (long long)batch * per_image * G;
    if ((threads + 255) / 256 > 0x7fffffffLL) return BRCNN_EINVAL;
    hipLaunchKernelGGL(cascade_refine_test_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0,
                       (hipStream_t)stream, dets, num, cls_score, cls_stride, bbox_pred, reg_stride, max_shape, batch,
                       per_image, num_classes, G, reg_class_agnostic ? 1 : 0, first ? 1 : 0, cd, dets_out, logit_sum);
    BRCNN_LAUNCH_CHECK();
    return 0;
}

BRCNN_API int brcnn_cascade_mean_softmax(const float* logit_sum, const float* cls_score_last, int cls_stride, int64_t rows,
                                         int num_classes, int num_stages, float* probs, float* mean_logits,
                                         void* stream) {
    if (!cls_score_last || !probs || rows < 0 || num_classes < 1 || num_stages < 1 || cls_stride < num_classes + 1 ||
        (num_stages > 1 && !logit_sum))
        return BRCNN_EINVAL;
    if (rows == 0) return 0;
    const int G = cascade_group(num_classes);
    const long long threads = (long long)rows * G;
    if ((threads + 255) / 256 > 0x7fffffffLL) return BRCNN_EINVAL;
    hipLaunchKernelGGL(cascade_mean_softmax_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0,
                       (hipStream_t)stream, num_stages > 1 ? logit_sum : nullptr, cls_score_last, cls_stride,
                       (long long)rows, num_classes, G, (float)num_stages, probs, mean_logits);
    BRCNN_LAUNCH_CHECK();
    return 0;
}

BRCNN_API int brcnn_cascade_refine_train(const float* rois, const int64_t* labels, const int32_t* gt_flags,
                                         const int* row_offsets_host, int batch, const float* cls_score, int cls_stride,
                                         const float* bbox_pred, int reg_stride, const float* max_shape, int num_classes,
                                         int reg_class_agnostic, const float* means4_host, const float* stds4_host,
                                         double wh_ratio_clip, int rows_out, float* props_out, int32_t* num_out,
                                         void* stream) {
    if (!row_offsets_host || batch <= 0 || batch > BRCNN_MAX_IMAGES || !max_shape || !props_out || !num_out ||
        num_classes < 1 || rows_out <= 0 || cls_stride < num_classes + 1 ||
        reg_stride < (reg_class_agnostic ? 4 : 4 * num_classes))
        return BRCNN_EINVAL;
    RefineTrainParams p;
    if (int st = fill_coder(p.cd, means4_host, stds4_host, wh_ratio_clip)) return st;
    if (row_offsets_host[0] < 0) return BRCNN_EINVAL;
    for (int b = 0; b <= batch; b++) {
        p.row0[b] = row_offsets_host[b];
        if (b) {
            const int rows = p.row0[b] - p.row0[b - 1];
            if (rows < 0 || rows > CASCADE_MAX_ROWS || rows > rows_out) return BRCNN_EINVAL;
        }
    }
    if (p.row0[batch] > 0 && (!rois || !labels || !gt_flags || !cls_score || !bbox_pred)) return BRCNN_EINVAL;
    p.rois = rois; p.labels = (const long long*)labels; p.gt_flags = gt_flags;
    p.cls = cls_score; p.reg = bbox_pred; p.cls_stride = cls_stride; p.reg_stride = reg_stride;
    p.max_shape = max_shape; p.C = num_classes; p.G = cascade_group(num_classes);
    p.agnostic = reg_class_agnostic ? 1 : 0; p.Kout = rows_out; p.props_out = props_out; p.num_out = num_out;
    hipLaunchKernelGGL(cascade_refine_train_kernel, dim3(batch), dim3(1024), 0, (hipStream_t)stream, p);
    BRCNN_LAUNCH_CHECK();
    return 0;
}
