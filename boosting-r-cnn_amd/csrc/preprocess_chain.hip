// Training front door of the multi-scale recipes: [RandomFlip ->] Resize -> RandomCrop -> Resize [-> RandomFlip] ->
// Normalize -> Pad of ONE decoded uint8 BGR image in one launch (the one-resize form and the arithmetic: preprocess.hip).
//   read  src  (H0, W0, 3) u8 HWC
//   write dst  (3, PH, PW) fp32 CHW, EVERY element: pixels, then zeros at the bottom / right
// Geometry.  Stage 1 resizes the source to a VIRTUAL (H1, W1) u8 image that is never stored; the window
// [top, top + ch) x [left, left + cw) of it is resized by stage 2 to (H2, W2).  Both stages are OpenCV's 8-bit
// INTER_LINEAR and both round to u8, so an output pixel is the stage-2 combination of 2 x 2 window pixels, each of which
// is the stage-1 combination of 2 x 2 source pixels: 16 taps x 3 bytes, all in registers.  Stage 2 clamps its taps to
// the WINDOW (a tap never reads the virtual image outside it), stage 1 to the source.  A stage whose sizes match is the
// identity under the same formula (coefficients 2048 / 0), as the host's copy is.
// `src_flip` mirrors the source before stage 1 (a RandomFlip in front of the policies), `flip` the (H2, W2) result (one
// behind them); resize and flip do not commute bit for bit, hence the two.
// Work split (preprocess_batch.hip): a workgroup owns a 64-row x 128-column tile; a lane owns 4 output columns, whose
// stage-2 and stage-1 x coefficients it derives once and reuses over its 8 rows.  With pad_w % 4 == 0 the 4 columns are
// consecutive and every plane gets one 16-byte store; otherwise (Pad(size_divisor=1) leaves rows of any length) they
// are 32 apart, so that each 4-byte store instruction of a half-wave still covers 128 contiguous bytes.  Lanes and rows
// of the padding region only store.
#include "common.h"

namespace {

constexpr int TILE_W = 128, TILE_H = 64, ROW_SLOTS = 8;

struct ChainParams {
    const uint8_t* src;
    float* dst;
    int h0, w0, h1, w1, top, left, ch, cw, h2, w2, ph, pw;
    int src_flip, flip, to_rgb, vec;
    double s1x, s1y, s2x, s2y;
    float mean[3], stdinv[3];
};

// (identical to preprocess.hip: the kernels must agree bit for bit)
__device__ __forceinline__ void axis_coeff(int d, double scale, int src, int& s, int& c0, int& c1) {
    float f = (float)(((double)d + 0.5) * scale - 0.5);
    s = (int)floorf(f);
    f -= (float)s;
    if (s < 0) { f = 0.f; s = 0; }
    if (s >= src - 1) { f = 0.f; s = src - 1; }
    c0 = (int)rintf((1.f - f) * 2048.f);
    c1 = (int)rintf(f * 2048.f);
}

// one axis of stage 1 for the virtual-image coordinate `v`: the two source indices (clamped, mirrored when `mirror`)
// and their coefficients
__device__ __forceinline__ void stage1_axis(int v, double scale, int n, bool mirror, int& i0, int& i1, int& c0, int& c1) {
    int s;
    axis_coeff(v, scale, n, s, c0, c1);
    i0 = min(max(s, 0), n - 1);
    i1 = min(max(s + 1, 0), n - 1);
    if (mirror) { i0 = n - 1 - i0; i1 = n - 1 - i1; }
}

__device__ __forceinline__ int combine(int p00, int p01, int p10, int p11, int a0, int a1, int b0, int b1) {
    const int h0 = p00 * a0 + p01 * a1, h1 = p10 * a0 + p11 * a1;
    const int q = (((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2;
    return min(max(q, 0), 255);
}

typedef float f32x4 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(256) void preprocess_u8_chain_kernel(ChainParams p) {
    const int lane = threadIdx.x & 31, slot = threadIdx.x >> 5;
    const int tx = blockIdx.x * TILE_W;
    const int y0 = blockIdx.y * TILE_H + slot;
    const int xbase = tx + (p.vec ? lane * 4 : lane), xstep = p.vec ? 1 : 32;
    if (xbase >= p.pw || y0 >= p.ph) return;
    const size_t plane = (size_t)p.ph * p.pw;
    const size_t row_bytes = (size_t)p.w0 * 3;

    // per column k: stage-2 coefficients a2, and per stage-2 tap t the stage-1 byte offsets / coefficients
    int a2[4][2], o1[4][2][2], a1[4][2][2];
    bool live[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int x = xbase + k * xstep;
        live[k] = x < p.w2;
        a2[k][0] = a2[k][1] = 0;
#pragma unroll
        for (int t = 0; t < 2; t++) o1[k][t][0] = o1[k][t][1] = a1[k][t][0] = a1[k][t][1] = 0;
        if (!live[k]) continue;
        int s;
        axis_coeff((p.flip & 1) ? p.w2 - 1 - x : x, p.s2x, p.cw, s, a2[k][0], a2[k][1]);
        const int wx[2] = {s, min(s + 1, p.cw - 1)};
#pragma unroll
        for (int t = 0; t < 2; t++) {
            int i0, i1;
            stage1_axis(p.left + wx[t], p.s1x, p.w0, p.src_flip & 1, i0, i1, a1[k][t][0], a1[k][t][1]);
            o1[k][t][0] = i0 * 3;
            o1[k][t][1] = i1 * 3;
        }
    }
    const int c_first = p.to_rgb ? 2 : 0, c_step = p.to_rgb ? -1 : 1;

#pragma unroll 1
    for (int y = y0; y < p.ph && y < y0 + TILE_H - slot; y += ROW_SLOTS) {
        float v[3][4];
#pragma unroll
        for (int c = 0; c < 3; c++)
#pragma unroll
            for (int k = 0; k < 4; k++) v[c][k] = 0.f;
        if (y < p.h2 && live[0]) {
            int s, b2[2], b1[2][2];
            const uint8_t* r[2][2];
            axis_coeff((p.flip & 2) ? p.h2 - 1 - y : y, p.s2y, p.ch, s, b2[0], b2[1]);
            const int wy[2] = {min(max(s, 0), p.ch - 1), min(max(s + 1, 0), p.ch - 1)};
#pragma unroll
            for (int t = 0; t < 2; t++) {
                int i0, i1;
                stage1_axis(p.top + wy[t], p.s1y, p.h0, p.src_flip & 2, i0, i1, b1[t][0], b1[t][1]);
                r[t][0] = p.src + (size_t)i0 * row_bytes;
                r[t][1] = p.src + (size_t)i1 * row_bytes;
            }
#pragma unroll
            for (int k = 0; k < 4; k++) {
                if (!live[k]) continue;
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    const int sc = c_first + c_step * c;
                    int w[2][2];                         // the 2 x 2 window pixels (rounded to u8) under this output pixel
#pragma unroll
                    for (int ty = 0; ty < 2; ty++)
#pragma unroll
                        for (int t = 0; t < 2; t++)
                            w[ty][t] = combine(r[ty][0][o1[k][t][0] + sc], r[ty][0][o1[k][t][1] + sc],
                                               r[ty][1][o1[k][t][0] + sc], r[ty][1][o1[k][t][1] + sc],
                                               a1[k][t][0], a1[k][t][1], b1[ty][0], b1[ty][1]);
                    const int q = combine(w[0][0], w[0][1], w[1][0], w[1][1], a2[k][0], a2[k][1], b2[0], b2[1]);
                    v[c][k] = ((float)q - p.mean[c]) * p.stdinv[c];
                }
            }
        }
        float* o = p.dst + (size_t)y * p.pw + xbase;
        if (p.vec) {
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const f32x4 q = {v[c][0], v[c][1], v[c][2], v[c][3]};
                *reinterpret_cast<f32x4*>(o + c * plane) = q;
            }
        } else {
#pragma unroll
            for (int k = 0; k < 4; k++) {
                if (xbase + k * 32 >= p.pw) break;
#pragma unroll
                for (int c = 0; c < 3; c++) o[c * plane + k * 32] = v[c][k];
            }
        }
    }
}

}  // namespace

BRCNN_API int brcnn_preprocess_u8_chain(const uint8_t* src, int src_h, int src_w, int src_flip, int mid_h, int mid_w,
                                        int top, int left, int crop_h, int crop_w, float* dst, int new_h, int new_w,
                                        int pad_h, int pad_w, int flip, const float* mean3_host,
                                        const float* std3_host, int to_rgb, void* stream) {
    if (!src || !dst || !mean3_host || !std3_host || src_h <= 0 || src_w <= 0 || mid_h <= 0 || mid_w <= 0 ||
        crop_h <= 0 || crop_w <= 0 || new_h <= 0 || new_w <= 0 || top < 0 || left < 0 || crop_h > mid_h - top ||
        crop_w > mid_w - left || pad_h < new_h || pad_w < new_w || flip < 0 || flip > 3 || src_flip < 0 ||
        src_flip > 3 || (int64_t)src_h * src_w * 3 > 0x7fffffff)
        return BRCNN_EINVAL;
    ChainParams p;
    p.src = src; p.dst = dst;
    p.h0 = src_h; p.w0 = src_w; p.h1 = mid_h; p.w1 = mid_w; p.top = top; p.left = left; p.ch = crop_h; p.cw = crop_w;
    p.h2 = new_h; p.w2 = new_w; p.ph = pad_h; p.pw = pad_w;
    p.src_flip = src_flip; p.flip = flip; p.to_rgb = to_rgb ? 1 : 0;
    p.vec = ((pad_w & 3) == 0 && ((uintptr_t)dst & 15) == 0) ? 1 : 0;
    p.s1x = 1.0 / ((double)mid_w / (double)src_w);
    p.s1y = 1.0 / ((double)mid_h / (double)src_h);
    p.s2x = 1.0 / ((double)new_w / (double)crop_w);
    p.s2y = 1.0 / ((double)new_h / (double)crop_h);
    for (int c = 0; c < 3; c++) {
        if (!(std3_host[c] != 0.f)) return BRCNN_EINVAL;
        p.mean[c] = mean3_host[c];
        p.stdinv[c] = (float)(1.0 / (double)std3_host[c]);
    }
    hipLaunchKernelGGL(preprocess_u8_chain_kernel, dim3((pad_w + TILE_W - 1) / TILE_W, (pad_h + TILE_H - 1) / TILE_H),
                       dim3(256), 0, (hipStream_t)stream, p);
    BRCNN_LAUNCH_CHECK();
    return 0;
}
