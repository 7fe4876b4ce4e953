// Res2Net-DCN rows of the hot path (configs/boosting_rcnn/boosting_rcnn_r2_101_*: Res2Net-101
// with DCNv2 in stages 2-4):
//   * average pooling of NHWC maps (res2net.py:52-54 AvgPool2d(3, stride, padding=1) on the last
//     split of a stage-opening block; res2net.py:173-178 AvgPool2d(stride, stride, ceil_mode=True,
//     count_include_pad=False) in the avg_down shortcut; resnet.py deep-stem variants),
//   * the modulated deformable im2col of mmcv's ModulatedDeformConv2dPack (mmcv 1.4.0
//     ops/csrc/common/cuda/modulated_deform_conv_cuda_kernel.cuh: dmcn_im2col_bilinear and
//     modulated_deformable_im2col_gpu_kernel), deform_groups = 1: column row m = (n, ho, wo),
//     column index (tap, c) -- the K order of this repo's packed weights -- so the GEMM that
//     follows is the ordinary MFMA linear kernel with its fused BN / ReLU epilogue.
// Both are HBM-bound streams, 16 bytes of channels per lane.
#include "common.h"
#include "deform_common.h"
#include "policy.h"

namespace {

// four channels of an NHWC map at element index i as fp32 (DT: BRCNN_DT_F32 / _BF16 / _F16), and back (one rounding)
template <int DT> __device__ __forceinline__ float4 ld4f(const void* p, size_t i) {
    if constexpr (DT == BRCNN_DT_F32) {
        return *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(p) + i);
    } else {
        const uint2 q = *reinterpret_cast<const uint2*>(reinterpret_cast<const unsigned short*>(p) + i);
        return make_float4(deform_e2f<DT>((unsigned short)q.x), deform_e2f<DT>((unsigned short)(q.x >> 16)),
                           deform_e2f<DT>((unsigned short)q.y), deform_e2f<DT>((unsigned short)(q.y >> 16)));
    }
}
template <int DT> __device__ __forceinline__ void st4f(void* p, size_t i, float4 v) {
    if constexpr (DT == BRCNN_DT_F32) {
        *reinterpret_cast<float4*>(reinterpret_cast<float*>(p) + i) = v;
    } else {
        uint2 q;
        q.x = DT == BRCNN_DT_F16 ? brcnn_pk2h(v.x, v.y) : brcnn_pk2b(v.x, v.y);
        q.y = DT == BRCNN_DT_F16 ? brcnn_pk2h(v.z, v.w) : brcnn_pk2b(v.z, v.w);
        *reinterpret_cast<uint2*>(reinterpret_cast<unsigned short*>(p) + i) = q;
    }
}

// fp32 sums and divisor in every element type; the 16-bit forms round the mean once
template <int DT>
__global__ __launch_bounds__(256) void avgpool_nhwc_kernel(const void* __restrict__ x, void* __restrict__ y,
                                                          int N, int H, int W, int C, int Ho, int Wo, int k,
                                                          int stride, int pad, int count_include_pad) {
    const int c4n = C >> 2;
    const long long total = (long long)N * Ho * Wo * c4n;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
         idx += (long long)gridDim.x * blockDim.x) {
        const int c4 = (int)(idx % c4n);
        long long r = idx / c4n;
        const int wo = (int)(r % Wo); r /= Wo;
        const int ho = (int)(r % Ho);
        const int n = (int)(r / Ho);
        // torch AvgPool2d window: [hs, he) clipped to the padded extent, divisor per count_include_pad
        int hs = ho * stride - pad, ws = wo * stride - pad;
        int he = min(hs + k, H + pad), we = min(ws + k, W + pad);
        const int pool_size = (he - hs) * (we - ws);
        hs = max(hs, 0); ws = max(ws, 0);
        he = min(he, H); we = min(we, W);
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int h = hs; h < he; h++)
            for (int w = ws; w < we; w++) {
                const float4 v = ld4f<DT>(x, (((size_t)n * H + h) * W + w) * C + c4 * 4);
                a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w;
            }
        const float div = (float)(count_include_pad ? pool_size : (he - hs) * (we - ws));
        a.x /= div; a.y /= div; a.z /= div; a.w /= div;
        st4f<DT>(y, (size_t)idx * 4, a);
    }
}

__device__ __forceinline__ float4 ld4z(const float* x, int H, int W, int C, int n, int h, int w, int c, bool ok) {
    if (!ok) return make_float4(0.f, 0.f, 0.f, 0.f);
    return *reinterpret_cast<const float4*>(x + (((size_t)n * H + h) * W + w) * C + c);
}

template <int DT>
__device__ __forceinline__ float4 ld4z_t(const void* x, int H, int W, int C, int n, int h, int w, int c, bool ok) {
    if (!ok) return make_float4(0.f, 0.f, 0.f, 0.f);
    return ld4f<DT>(x, (((size_t)n * H + h) * W + w) * C + c);
}

// one thread: one (output pixel, tap, 4 channels)
__global__ __launch_bounds__(256) void deform_im2col_nhwc_kernel(const float* __restrict__ x,
                                                                const float* __restrict__ om,
                                                                float* __restrict__ col, int N, int H, int W,
                                                                int C, int Ho, int Wo, int KH, int KW, int stride,
                                                                int pad, int dilation, int om_stride, int Cpad, int G,
                                                                int modulated) {
    // deform groups: channel c takes the offsets (and mask logit) of group c / (C / G); the offset row of a pixel is
    // [2 T g + 2 t] dy, [2 T g + 2 t + 1] dx, [2 T G + T g + t] mask logit (modulated only; v1: the factor is 1)
    const int c4n = Cpad >> 2, taps = KH * KW, cg = C / G;
    const long long total = (long long)N * Ho * Wo * taps * c4n;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
         idx += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(idx % c4n) * 4;
        long long r = idx / c4n;
        const int tap = (int)(r % taps); r /= taps;
        const long long m = r;
        const int wo = (int)(m % Wo);
        const int ho = (int)((m / Wo) % Ho);
        const int n = (int)(m / ((long long)Wo * Ho));
        float4 out = make_float4(0.f, 0.f, 0.f, 0.f);
        if (c < C) {
            const int i = tap / KW, j = tap - i * KW;
            const float* o = om + (size_t)m * om_stride;
            const int grp = c / cg;
            const float off_h = o[2 * taps * grp + 2 * tap], off_w = o[2 * taps * grp + 2 * tap + 1];
            const float mask = modulated ? 1.f / (1.f + expf(-o[2 * taps * G + taps * grp + tap])) : 1.f;
            const float h_im = (float)(ho * stride - pad + i * dilation) + off_h;
            const float w_im = (float)(wo * stride - pad + j * dilation) + off_w;
            if (h_im > -1.f && w_im > -1.f && h_im < (float)H && w_im < (float)W) {
                const int h_low = (int)floorf(h_im), w_low = (int)floorf(w_im);
                const int h_high = h_low + 1, w_high = w_low + 1;
                const float lh = h_im - (float)h_low, lw = w_im - (float)w_low;
                const float hh = 1.f - lh, hw = 1.f - lw;
                const float4 v1 = ld4z(x, H, W, C, n, h_low, w_low, c, h_low >= 0 && w_low >= 0);
                const float4 v2 = ld4z(x, H, W, C, n, h_low, w_high, c, h_low >= 0 && w_high <= W - 1);
                const float4 v3 = ld4z(x, H, W, C, n, h_high, w_low, c, h_high <= H - 1 && w_low >= 0);
                const float4 v4 = ld4z(x, H, W, C, n, h_high, w_high, c, h_high <= H - 1 && w_high <= W - 1);
                const float w1 = hh * hw, w2 = hh * lw, w3 = lh * hw, w4 = lh * lw;
                out.x = (w1 * v1.x + w2 * v2.x + w3 * v3.x + w4 * v4.x) * mask;
                out.y = (w1 * v1.y + w2 * v2.y + w3 * v3.y + w4 * v4.y) * mask;
                out.z = (w1 * v1.z + w2 * v2.z + w3 * v3.z + w4 * v4.z) * mask;
                out.w = (w1 * v1.w + w2 * v2.w + w3 * v3.w + w4 * v4.w) * mask;
            }
        }
        *reinterpret_cast<float4*>(col + (size_t)idx * 4) = out;
    }
}

// Backward of the modulated deformable im2col (mmcv modulated_deformable_col2im_gpu_kernel and
// modulated_deformable_col2im_coord_gpu_kernel): one wavefront per (output pixel, tap, deform group), lanes over
// the group's channels.  dx gets dcol * mask * corner weight (fp32 atomics, like the RoIAlign backward); the
// offset / mask gradients are channel sums, reduced across the wave and written once:
//   d off_h = mask * sum_c dcol_c * d val_c / d h,   d off_w likewise,
//   d mask_logit = mask (1 - mask) * sum_c dcol_c * val_c          (sigmoid applied in the forward)
// (16-bit x: the same arithmetic on the widened corners; dx stays an fp32 accumulator the caller converts)
// ORDERED: dx is a table of 64-bit integers and a contribution is added as an integer -- integer addition is associative,
// so the sums (and, after dx_fixed_to_f32_kernel, dx) carry the same bits from run to run, which fp32 atomics in whatever
// order the waves arrive do not.  The grid is chosen from the data of the call: a pre-pass takes m = max |dcol| (a maximum
// does not depend on the order either) and its binary exponent ex (m < 2^ex); a contribution dcol * mask * corner weight is
// at most m in magnitude (mask and weight lie in [0, 1]) and is scaled by 2^(S - ex), S = 62 - ceil(log2(Ho Wo taps 4)): even
// if every sample of an image fell on one pixel the sum stays below 2^62, so nothing can overflow.  What it costs: each
// contribution is rounded to a multiple of 2^(ex - S) <= 2 m 2^-S (S = 41 for a 100 x 168 map, 50 for 6 x 7), i.e. an
// absolute error of at most m 2^-S per contribution whatever its size; a contribution of at least m 2^(24 - S) keeps the
// full 24 bits of fp32, one below m 2^-S-1 is dropped.  The two words behind the table hold the bits of m and the shift
// S - ex; a dcol or a contribution that is not finite sets the shift to ORDERED_POISON and the whole of dx reads NaN, so that
// an overflowed fp16 step is still seen as one.
constexpr int ORDERED_POISON = -2147483647 - 1;

__global__ __launch_bounds__(256) void dx_ordered_max_kernel(const float* __restrict__ dcol, long long n,
                                                            unsigned* __restrict__ tail) {
    unsigned m = 0u;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        m = max(m, __float_as_uint(dcol[i]) & 0x7fffffffu);       // |v| as bits: ordered like the values, NaN above inf
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, d));
    if ((threadIdx.x & 63) == 0 && m) atomicMax(tail, m);
}

// tail[1] = S - ex, or ORDERED_POISON when max |dcol| is not finite
__global__ void dx_ordered_shift_kernel(int* __restrict__ tail, int S) {
    const unsigned bits = (unsigned)tail[0];
    int ex = 0;
    frexpf(__uint_as_float(bits), &ex);
    tail[1] = bits >= 0x7f800000u ? ORDERED_POISON : S - ex;
}

template <bool ORDERED>
__device__ __forceinline__ void dx_add(float* dx, size_t i, float v, int* tail) {
    if (ORDERED) {
        const int shift = tail[1];
        if (shift == ORDERED_POISON) return;
        if (!isfinite(v)) { atomicMin(tail + 1, ORDERED_POISON); return; }
        atomicAdd(reinterpret_cast<unsigned long long*>(dx) + i, (unsigned long long)__double2ll_rn(ldexp((double)v, shift)));
    } else {
        atomicAdd(dx + i, v);
    }
}

__global__ __launch_bounds__(256) void dx_fixed_to_f32_kernel(const long long* __restrict__ acc, float* __restrict__ dx,
                                                             long long n) {
    const int shift = reinterpret_cast<const int*>(acc + n)[1];
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        dx[i] = shift == ORDERED_POISON ? __builtin_nanf("") : (float)ldexp((double)acc[i], -shift);
}

template <int DT, bool ORDERED = false>
__global__ __launch_bounds__(256) void deform_col2im_nhwc_kernel(const void* __restrict__ x,
                                                                const float* __restrict__ om,
                                                                const float* __restrict__ dcol,
                                                                float* __restrict__ dx, float* __restrict__ dom,
                                                                int N, int H, int W, int C, int Ho, int Wo, int KH,
                                                                int KW, int stride, int pad, int dilation,
                                                                int om_stride, int Cpad, int G, int modulated) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int taps = KH * KW, cg = C / G;
    const long long item = (long long)blockIdx.x * 4 + wave;
    if (item >= (long long)N * Ho * Wo * taps * G) return;
    const int grp = (int)(item % G);
    const long long mt = item / G;
    const int tap = (int)(mt % taps);
    const long long m = mt / taps;
    const int wo = (int)(m % Wo);
    const int ho = (int)((m / Wo) % Ho);
    const int n = (int)(m / ((long long)Wo * Ho));
    const int i = tap / KW, j = tap - i * KW;
    const float* o = om + (size_t)m * om_stride;
    const float off_h = o[2 * taps * grp + 2 * tap], off_w = o[2 * taps * grp + 2 * tap + 1];
    const float mask = modulated ? 1.f / (1.f + expf(-o[2 * taps * G + taps * grp + tap])) : 1.f;
    const float h_im = (float)(ho * stride - pad + i * dilation) + off_h;
    const float w_im = (float)(wo * stride - pad + j * dilation) + off_w;
    const bool inside = h_im > -1.f && w_im > -1.f && h_im < (float)H && w_im < (float)W;
    int* bad = ORDERED ? reinterpret_cast<int*>(reinterpret_cast<long long*>(dx) + (size_t)N * H * W * C) : nullptr;    // the tail
    float g_h = 0.f, g_w = 0.f, g_m = 0.f;
    if (inside) {
        const int h_low = (int)floorf(h_im), w_low = (int)floorf(w_im);
        const int h_high = h_low + 1, w_high = w_low + 1;
        const float lh = h_im - (float)h_low, lw = w_im - (float)w_low;
        const float hh = 1.f - lh, hw = 1.f - lw;
        const bool ok1 = h_low >= 0 && w_low >= 0, ok2 = h_low >= 0 && w_high <= W - 1;
        const bool ok3 = h_high <= H - 1 && w_low >= 0, ok4 = h_high <= H - 1 && w_high <= W - 1;
        const float* dc = dcol + ((size_t)m * taps + tap) * Cpad;
        for (int c = grp * cg + lane * 4; c < (grp + 1) * cg; c += 256) {
            const float4 g = *reinterpret_cast<const float4*>(dc + c);
            const float4 v1 = ld4z_t<DT>(x, H, W, C, n, h_low, w_low, c, ok1);
            const float4 v2 = ld4z_t<DT>(x, H, W, C, n, h_low, w_high, c, ok2);
            const float4 v3 = ld4z_t<DT>(x, H, W, C, n, h_high, w_low, c, ok3);
            const float4 v4 = ld4z_t<DT>(x, H, W, C, n, h_high, w_high, c, ok4);
            const float gg[4] = {g.x, g.y, g.z, g.w};
            const float a1[4] = {v1.x, v1.y, v1.z, v1.w}, a2[4] = {v2.x, v2.y, v2.z, v2.w};
            const float a3[4] = {v3.x, v3.y, v3.z, v3.w}, a4[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const float val = hh * hw * a1[e] + hh * lw * a2[e] + lh * hw * a3[e] + lh * lw * a4[e];
                g_m += gg[e] * val;
                g_h += gg[e] * (-hw * a1[e] - lw * a2[e] + hw * a3[e] + lw * a4[e]);
                g_w += gg[e] * (-hh * a1[e] + hh * a2[e] - lh * a3[e] + lh * a4[e]);
                const float gx = gg[e] * mask;
                if (ok1) dx_add<ORDERED>(dx, (((size_t)n * H + h_low) * W + w_low) * C + c + e, gx * hh * hw, bad);
                if (ok2) dx_add<ORDERED>(dx, (((size_t)n * H + h_low) * W + w_high) * C + c + e, gx * hh * lw, bad);
                if (ok3) dx_add<ORDERED>(dx, (((size_t)n * H + h_high) * W + w_low) * C + c + e, gx * lh * hw, bad);
                if (ok4) dx_add<ORDERED>(dx, (((size_t)n * H + h_high) * W + w_high) * C + c + e, gx * lh * lw, bad);
            }
        }
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        g_h += __shfl_xor(g_h, d);
        g_w += __shfl_xor(g_w, d);
        g_m += __shfl_xor(g_m, d);
    }
    if (lane == 0) {
        float* go = dom + (size_t)m * om_stride;
        go[2 * taps * grp + 2 * tap] = g_h * mask;
        go[2 * taps * grp + 2 * tap + 1] = g_w * mask;
        if (modulated) go[2 * taps * G + taps * grp + tap] = g_m * mask * (1.f - mask);
    }
}

// 16-bit im2col: one thread per (output pixel, tap, 8 channels); the sample comes from deform_sample8, the routine
// the fused conv (deform_conv_bf16.hip) builds its A operand with.  Corner loads from clamped addresses, unconditional.
template <int DT>
__global__ __launch_bounds__(256) void deform_im2col_nhwc16_kernel(const unsigned short* __restrict__ x,
                                                                  const float* __restrict__ om,
                                                                  unsigned short* __restrict__ col, int N, int H, int W,
                                                                  int C, int Ho, int Wo, int KH, int KW, int stride,
                                                                  int pad, int dilation, int om_stride, int Cpad, int G,
                                                                  int modulated) {
    const int c8n = Cpad >> 3, taps = KH * KW, cg = C / G;      // cg % 8 == 0: a thread's eight channels share a group
    const long long total = (long long)N * Ho * Wo * taps * c8n;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
         idx += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(idx % c8n) * 8;
        long long r = idx / c8n;
        const int tap = (int)(r % taps); r /= taps;
        const long long m = r;
        const int wo = (int)(m % Wo);
        const int ho = (int)((m / Wo) % Ho);
        const int n = (int)(m / ((long long)Wo * Ho));
        const int i = tap / KW, j = tap - i * KW;
        const float* o = om + (size_t)m * om_stride;
        const int grp = c < C ? c / cg : 0;                     // (a pad channel belongs to no group: it reads group 0's row and stays 0)
        const float lg = modulated ? o[2 * taps * G + taps * grp + tap] : 0.f;
        const DeformTapGeom g = deform_tap_geom(o[2 * taps * grp + 2 * tap], o[2 * taps * grp + 2 * tap + 1], lg,
                                                ho * stride - pad + i * dilation, wo * stride - pad + j * dilation, H, W, C, c < C,
                                                modulated != 0);
        const unsigned short* xc = x + (size_t)n * H * W * C + (c < C ? c : 0);
        const uint4 v1 = *reinterpret_cast<const uint4*>(xc + g.off1);
        const uint4 v2 = *reinterpret_cast<const uint4*>(xc + g.off2);
        const uint4 v3 = *reinterpret_cast<const uint4*>(xc + g.off3);
        const uint4 v4 = *reinterpret_cast<const uint4*>(xc + g.off4);
        *reinterpret_cast<uint4*>(col + (size_t)idx * 8) = deform_sample8<DT>(g, v1, v2, v3, v4);
    }
}

// torch AvgPool2d output size (the last window must start inside the input in ceil mode)
// (the division rounds towards minus infinity, as torch's does: a map smaller than the window has no output, where
// C's truncation would give it one)
inline int brcnn_avgpool_out(int in, int kernel, int stride, int pad, int ceil_mode) {
    const int num = in + 2 * pad - kernel + (ceil_mode ? stride - 1 : 0);
    if (num < 0) return 0;
    int o = num / stride + 1;
    if (ceil_mode && (o - 1) * stride >= in + pad) o--;
    return o;
}

// a kernel extent the padded map does not hold has no output either (C's truncating division would give it one row)
inline bool deform_out_size(int height, int width, int kh, int kw, int stride, int pad, int dilation, int* Ho, int* Wo) {
    const int eh = height + 2 * pad - (dilation * (kh - 1) + 1), ew = width + 2 * pad - (dilation * (kw - 1) + 1);
    if (eh < 0 || ew < 0) return false;
    *Ho = eh / stride + 1;
    *Wo = ew / stride + 1;
    return true;
}

inline int stream_grid(long long total) {
    long long g = (total + 255) / 256;
    return (int)(g > 32768 ? 32768 : (g < 1 ? 1 : g));
}

}  // namespace

BRCNN_API int brcnn_avgpool_nhwc(const float* x, float* y, int batch, int height, int width, int channels,
                                 int kernel, int stride, int pad, int ceil_mode, int count_include_pad,
                                 void* stream) {
    if (!x || !y || batch <= 0 || height <= 0 || width <= 0 || channels <= 0 || (channels & 3) || kernel <= 0 ||
        stride <= 0 || pad < 0 || pad > kernel / 2)
        return BRCNN_EINVAL;
    const int Ho = brcnn_avgpool_out(height, kernel, stride, pad, ceil_mode);
    const int Wo = brcnn_avgpool_out(width, kernel, stride, pad, ceil_mode);
    if (Ho <= 0 || Wo <= 0) return BRCNN_EINVAL;
    const long long total = (long long)batch * Ho * Wo * (channels >> 2);
    hipLaunchKernelGGL(avgpool_nhwc_kernel<BRCNN_DT_F32>, dim3(stream_grid(total)), dim3(256), 0, (hipStream_t)stream, x, y, batch,
                       height, width, channels, Ho, Wo, kernel, stride, pad, count_include_pad);
    BRCNN_LAUNCH_CHECK();
    return 0;
}

BRCNN_API int brcnn_deform_im2col_nhwc(const float* x, const float* offset_mask, float* col, int batch,
                                       int height, int width, int channels, int kh, int kw, int stride, int pad,
                                       int dilation, int om_stride, int channels_padded, void* stream) {
    if (!x || !offset_mask || !col || batch <= 0 || height <= 0 || width <= 0 || channels <= 0 || (channels & 3) ||
        kh <= 0 || kw <= 0 || stride <= 0 || pad < 0 || dilation <= 0 || om_stride < 3 * kh * kw ||
        channels_padded < channels || (channels_padded & 3))
        return BRCNN_EINVAL;
    int Ho, Wo;
    if (!deform_out_size(height, width, kh, kw, stride, pad, dilation, &Ho, &Wo)) return BRCNN_EINVAL;
    const long long total = (long long)batch * Ho * Wo * kh * kw * (channels_padded >> 2);
    hipLaunchKernelGGL(deform_im2col_nhwc_kernel, dim3(stream_grid(total)), dim3(256), 0, (hipStream_t)stream, x,
                       offset_mask, col, batch, height, width, channels, Ho, Wo, kh, kw, stride, pad, dilation,
                       om_stride, channels_padded, 1, 1);
    BRCNN_LAUNCH_CHECK();
    brcnn::count(brcnn::g_counters.dcn_im2col_launches);
    return 0;
}


BRCNN_API int brcnn_deform_col2im_nhwc(const float* x, const float* offset_mask, const float* dcol, float* dx,
                                       float* d_offset_mask, int batch, int height, int width, int channels,
                                       int kh, int kw, int stride, int pad, int dilation, int om_stride,
                                       int channels_padded, void* stream) {
    if (!x || !offset_mask || !dcol || !dx || !d_offset_mask || batch <= 0 || height <= 0 || width <= 0 ||
        channels <= 0 || (channels & 3) || kh <= 0 || kw <= 0 || stride <= 0 || pad < 0 || dilation <= 0 ||
        om_stride != 3 * kh * kw || channels_padded < channels || (channels_padded & 3))
        return BRCNN_EINVAL;
    int Ho, Wo;
    if (!deform_out_size(height, width, kh, kw, stride, pad, dilation, &Ho, &Wo)) return BRCNN_EINVAL;
    const long long items = (long long)batch * Ho * Wo * kh * kw;
    hipLaunchKernelGGL(deform_col2im_nhwc_kernel<BRCNN_DT_F32>, dim3((unsigned)((items + 3) / 4)), dim3(256), 0, (hipStream_t)stream,
                       x, offset_mask, dcol, dx, d_offset_mask, batch, height, width, channels, Ho, Wo, kh, kw, stride,
                       pad, dilation, om_stride, channels_padded, 1, 1);
    BRCNN_LAUNCH_CHECK();
    return 0;
}


// ---- 16-bit forms (bf16 / fp16 activations; the offsets / mask logits and every gradient stay fp32) ----------------
BRCNN_API int brcnn_avgpool_nhwc_ex(const void* x, void* y, int batch, int height, int width, int channels, int kernel,
                                    int stride, int pad, int ceil_mode, int count_include_pad, int dtype, void* stream) {
    if (dtype == BRCNN_DT_F32)
        return brcnn_avgpool_nhwc((const float*)x, (float*)y, batch, height, width, channels, kernel, stride, pad, ceil_mode,
                                  count_include_pad, stream);
    if (!x || !y || batch <= 0 || height <= 0 || width <= 0 || channels <= 0 || (channels & 3) || kernel <= 0 ||
        stride <= 0 || pad < 0 || pad > kernel / 2 || (dtype != BRCNN_DT_BF16 && dtype != BRCNN_DT_F16))
        return BRCNN_EINVAL;
    const int Ho = (int)brcnn_avgpool_out(height, kernel, stride, pad, ceil_mode);
    const int Wo = (int)brcnn_avgpool_out(width, kernel, stride, pad, ceil_mode);
    if (Ho <= 0 || Wo <= 0) return BRCNN_EINVAL;
    const long long total = (long long)batch * Ho * Wo * (channels >> 2);
    if (dtype == BRCNN_DT_F16)
        hipLaunchKernelGGL(avgpool_nhwc_kernel<BRCNN_DT_F16>, dim3(stream_grid(total)), dim3(256), 0, (hipStream_t)stream, x,
                           y, batch, height, width, channels, Ho, Wo, kernel, stride, pad, count_include_pad);
    else
        hipLaunchKernelGGL(avgpool_nhwc_kernel<BRCNN_DT_BF16>, dim3(stream_grid(total)), dim3(256), 0, (hipStream_t)stream, x,
                           y, batch, height, width, channels, Ho, Wo, kernel, stride, pad, count_include_pad);
    BRCNN_LAUNCH_CHECK();
    return 0;
}

BRCNN_API int brcnn_deform_im2col_nhwc_ex(const void* x, const float* offset_mask, void* col, int batch, int height,
                                          int width, int channels, int kh, int kw, int stride, int pad, int dilation,
                                          int om_stride, int channels_padded, int dtype, void* stream) {
    if (dtype == BRCNN_DT_F32)
        return brcnn_deform_im2col_nhwc((const float*)x, offset_mask, (float*)col, batch, height, width, channels, kh, kw,
                                        stride, pad, dilation, om_stride, channels_padded, stream);
    if (!x || !offset_mask || !col || batch <= 0 || height <= 0 || width <= 0 || channels <= 0 || (channels & 7) ||
        kh <= 0 || kw <= 0 || stride <= 0 || pad < 0 || dilation <= 0 || om_stride < 3 * kh * kw ||
        channels_padded < channels || (channels_padded & 7) || (dtype != BRCNN_DT_BF16 && dtype != BRCNN_DT_F16) ||
        (long long)batch * height * width * channels >= 0x7fffffffLL)
        return BRCNN_EINVAL;
    int Ho, Wo;
    if (!deform_out_size(height, width, kh, kw, stride, pad, dilation, &Ho, &Wo)) return BRCNN_EINVAL;
    const long long total = (long long)batch * Ho * Wo * kh * kw * (channels_padded >> 3);
    if (dtype == BRCNN_DT_F16)
        hipLaunchKernelGGL(deform_im2col_nhwc16_kernel<BRCNN_DT_F16>, dim3(stream_grid(total)), dim3(256), 0,
                           (hipStream_t)stream, (const unsigned short*)x, offset_mask, (unsigned short*)col, batch, height,
                           width, channels, Ho, Wo, kh, kw, stride, pad, dilation, om_stride, channels_padded, 1, 1);
    else
        hipLaunchKernelGGL(deform_im2col_nhwc16_kernel<BRCNN_DT_BF16>, dim3(stream_grid(total)), dim3(256), 0,
                           (hipStream_t)stream, (const unsigned short*)x, offset_mask, (unsigned short*)col, batch, height,
                           width, channels, Ho, Wo, kh, kw, stride, pad, dilation, om_stride, channels_padded, 1, 1);
    BRCNN_LAUNCH_CHECK();
    brcnn::count(brcnn::g_counters.dcn_im2col_launches);
    return 0;
}

BRCNN_API int brcnn_deform_col2im_nhwc_ex(const void* x, const float* offset_mask, const float* dcol, float* dx,
                                          float* d_offset_mask, int batch, int height, int width, int channels, int kh,
                                          int kw, int stride, int pad, int dilation, int om_stride, int channels_padded,
                                          int dtype, void* stream) {
    if (dtype == BRCNN_DT_F32)
        return brcnn_deform_col2im_nhwc((const float*)x, offset_mask, dcol, dx, d_offset_mask, batch, height, width,
                                        channels, kh, kw, stride, pad, dilation, om_stride, channels_padded, stream);
    if (!x || !offset_mask || !dcol || !dx || !d_offset_mask || batch <= 0 || height <= 0 || width <= 0 ||
        channels <= 0 || (channels & 3) || kh <= 0 || kw <= 0 || stride <= 0 || pad < 0 || dilation <= 0 ||
        om_stride != 3 * kh * kw || channels_padded < channels || (channels_padded & 3) ||
        (dtype != BRCNN_DT_BF16 && dtype != BRCNN_DT_F16))
        return BRCNN_EINVAL;
    int Ho, Wo;
    if (!deform_out_size(height, width, kh, kw, stride, pad, dilation, &Ho, &Wo)) return BRCNN_EINVAL;
    const long long items = (long long)batch * Ho * Wo * kh * kw;
    if (dtype == BRCNN_DT_F16)
        hipLaunchKernelGGL(deform_col2im_nhwc_kernel<BRCNN_DT_F16>, dim3((unsigned)((items + 3) / 4)), dim3(256), 0,
                           (hipStream_t)stream, x, offset_mask, dcol, dx, d_offset_mask, batch, height, width, channels, Ho,
                           Wo, kh, kw, stride, pad, dilation, om_stride, channels_padded, 1, 1);
    else
        hipLaunchKernelGGL(deform_col2im_nhwc_kernel<BRCNN_DT_BF16>, dim3((unsigned)((items + 3) / 4)), dim3(256), 0,
                           (hipStream_t)stream, x, offset_mask, dcol, dx, d_offset_mask, batch, height, width, channels, Ho,
                           Wo, kh, kw, stride, pad, dilation, om_stride, channels_padded, 1, 1);
    BRCNN_LAUNCH_CHECK();
    return 0;
}

// ---- deform groups and the unmodulated form (DCN v1): offset rows of (modulated ? 3 : 2) * KH * KW * deform_groups floats
// in the layout of deform_im2col_nhwc_kernel; the entries above are these with deform_groups 1, modulated 1 ---------------
namespace {
bool deform_g_args_ok(const void* x, const float* om, int batch, int height, int width, int channels, int kh, int kw,
                      int stride, int pad, int dilation, int channels_padded, int groups, int modulated, int dtype) {
    if (!x || !om || batch <= 0 || height <= 0 || width <= 0 || channels <= 0 || kh <= 0 || kw <= 0 || stride <= 0 ||
        pad < 0 || dilation <= 0 || channels_padded < channels || groups <= 0 || channels % groups ||
        (modulated != 0 && modulated != 1) || (long long)kh * kw * groups > 4096)
        return false;
    if (dtype != BRCNN_DT_F32 && dtype != BRCNN_DT_BF16 && dtype != BRCNN_DT_F16) return false;
    // a thread's 4 (fp32) / 8 (16-bit) channels lie inside one group
    const int q = dtype == BRCNN_DT_F32 ? 3 : 7;
    return !((channels / groups) & q) && !(channels_padded & q);
}
}  // namespace

BRCNN_API int brcnn_deform_im2col_nhwc_g(const void* x, const float* offset_mask, void* col, int batch, int height,
                                         int width, int channels, int kh, int kw, int stride, int pad, int dilation,
                                         int om_stride, int channels_padded, int deform_groups, int modulated, int dtype,
                                         void* stream) {
    if (!col || !deform_g_args_ok(x, offset_mask, batch, height, width, channels, kh, kw, stride, pad, dilation,
                                  channels_padded, deform_groups, modulated, dtype))
        return BRCNN_EINVAL;
    if (om_stride < (modulated ? 3 : 2) * kh * kw * deform_groups) return BRCNN_EINVAL;
    if (dtype != BRCNN_DT_F32 && (long long)batch * height * width * channels >= 0x7fffffffLL) return BRCNN_EINVAL;
    int Ho, Wo;
    if (!deform_out_size(height, width, kh, kw, stride, pad, dilation, &Ho, &Wo)) return BRCNN_EINVAL;
    const long long total = (long long)batch * Ho * Wo * kh * kw * (channels_padded >> (dtype == BRCNN_DT_F32 ? 2 : 3));
    hipStream_t s = (hipStream_t)stream;
    if (dtype == BRCNN_DT_F32)
        hipLaunchKernelGGL(deform_im2col_nhwc_kernel, dim3(stream_grid(total)), dim3(256), 0, s, (const float*)x, offset_mask,
                           (float*)col, batch, height, width, channels, Ho, Wo, kh, kw, stride, pad, dilation, om_stride,
                           channels_padded, deform_groups, modulated);
    else if (dtype == BRCNN_DT_F16)
        hipLaunchKernelGGL(deform_im2col_nhwc16_kernel<BRCNN_DT_F16>, dim3(stream_grid(total)), dim3(256), 0, s,
                           (const unsigned short*)x, offset_mask, (unsigned short*)col, batch, height, width, channels, Ho, Wo,
                           kh, kw, stride, pad, dilation, om_stride, channels_padded, deform_groups, modulated);
    else
        hipLaunchKernelGGL(deform_im2col_nhwc16_kernel<BRCNN_DT_BF16>, dim3(stream_grid(total)), dim3(256), 0, s,
                           (const unsigned short*)x, offset_mask, (unsigned short*)col, batch, height, width, channels, Ho, Wo,
                           kh, kw, stride, pad, dilation, om_stride, channels_padded, deform_groups, modulated);
    BRCNN_LAUNCH_CHECK();
    brcnn::count(brcnn::g_counters.dcn_im2col_launches);
    return 0;
}

BRCNN_API int brcnn_deform_col2im_nhwc_g(const void* x, const float* offset_mask, const float* dcol, float* dx,
                                         float* d_offset_mask, int batch, int height, int width, int channels, int kh,
                                         int kw, int stride, int pad, int dilation, int om_stride, int channels_padded,
                                         int deform_groups, int modulated, int dtype, void* stream) {
    if (!dcol || !dx || !d_offset_mask ||
        !deform_g_args_ok(x, offset_mask, batch, height, width, channels, kh, kw, stride, pad, dilation, channels_padded,
                          deform_groups, modulated, dtype))
        return BRCNN_EINVAL;
    // every entry of a d_offset_mask row is written: the row is exactly the layout
    if (om_stride != (modulated ? 3 : 2) * kh * kw * deform_groups) return BRCNN_EINVAL;
    int Ho, Wo;
    if (!deform_out_size(height, width, kh, kw, stride, pad, dilation, &Ho, &Wo)) return BRCNN_EINVAL;
    const long long items = (long long)batch * Ho * Wo * kh * kw * deform_groups;
    if ((items + 3) / 4 >= 0x7fffffffLL) return BRCNN_EINVAL;
    const dim3 grid((unsigned)((items + 3) / 4));
    hipStream_t s = (hipStream_t)stream;
    if (dtype == BRCNN_DT_F32)
        hipLaunchKernelGGL(deform_col2im_nhwc_kernel<BRCNN_DT_F32>, grid, dim3(256), 0, s, x, offset_mask, dcol, dx,
                           d_offset_mask, batch, height, width, channels, Ho, Wo, kh, kw, stride, pad, dilation, om_stride,
                           channels_padded, deform_groups, modulated);
    else if (dtype == BRCNN_DT_F16)
        hipLaunchKernelGGL(deform_col2im_nhwc_kernel<BRCNN_DT_F16>, grid, dim3(256), 0, s, x, offset_mask, dcol, dx,
                           d_offset_mask, batch, height, width, channels, Ho, Wo, kh, kw, stride, pad, dilation, om_stride,
                           channels_padded, deform_groups, modulated);
    else
        hipLaunchKernelGGL(deform_col2im_nhwc_kernel<BRCNN_DT_BF16>, grid, dim3(256), 0, s, x, offset_mask, dcol, dx,
                           d_offset_mask, batch, height, width, channels, Ho, Wo, kh, kw, stride, pad, dilation, om_stride,
                           channels_padded, deform_groups, modulated);
    BRCNN_LAUNCH_CHECK();
    return 0;
}

// brcnn_deform_col2im_nhwc_g with dx accumulated in integers (ORDERED above): the same bits from run to run.  workspace:
// 8 bytes per element of dx and the two tail words; every element of dx is written
BRCNN_API size_t brcnn_deform_col2im_ordered_workspace_bytes(int batch, int height, int width, int channels) {
    if (batch <= 0 || height <= 0 || width <= 0 || channels <= 0) return 0;
    return ((size_t)batch * height * width * channels + 1) * sizeof(long long);      // + the tail: bits of max |dcol|, shift
}

BRCNN_API int brcnn_deform_col2im_nhwc_ordered(const void* x, const float* offset_mask, const float* dcol, float* dx,
                                               float* d_offset_mask, int batch, int height, int width, int channels, int kh,
                                               int kw, int stride, int pad, int dilation, int om_stride, int channels_padded,
                                               int deform_groups, int modulated, int dtype, void* workspace,
                                               size_t workspace_bytes, void* stream) {
    if (!dcol || !dx || !d_offset_mask || !workspace ||
        !deform_g_args_ok(x, offset_mask, batch, height, width, channels, kh, kw, stride, pad, dilation, channels_padded,
                          deform_groups, modulated, dtype))
        return BRCNN_EINVAL;
    if (om_stride != (modulated ? 3 : 2) * kh * kw * deform_groups) return BRCNN_EINVAL;
    const size_t need = brcnn_deform_col2im_ordered_workspace_bytes(batch, height, width, channels);
    if (!need || workspace_bytes < need) return BRCNN_EINVAL;
    int Ho, Wo;
    if (!deform_out_size(height, width, kh, kw, stride, pad, dilation, &Ho, &Wo)) return BRCNN_EINVAL;
    const long long items = (long long)batch * Ho * Wo * kh * kw * deform_groups;
    if ((items + 3) / 4 >= 0x7fffffffLL) return BRCNN_EINVAL;
    const dim3 grid((unsigned)((items + 3) / 4));
    hipStream_t s = (hipStream_t)stream;
    BRCNN_HIP_CHECK(hipMemsetAsync(workspace, 0, need, s));
    float* acc = reinterpret_cast<float*>(workspace);
    const long long n = (long long)batch * height * width * channels;
    int* tail = reinterpret_cast<int*>(reinterpret_cast<long long*>(workspace) + n);
    // S: the sum of every sample of one image on one pixel, Ho Wo taps 4 contributions below 2^S each, stays below 2^62
    const long long pile = (long long)Ho * Wo * kh * kw * 4;
    int hb = 0;
    while ((1LL << hb) < pile) hb++;
    const long long n_dcol = (long long)batch * Ho * Wo * kh * kw * channels_padded;
    long long gm = (n_dcol + 255) / 256;
    if (gm > 4096) gm = 4096;
    hipLaunchKernelGGL(dx_ordered_max_kernel, dim3((unsigned)gm), dim3(256), 0, s, dcol, n_dcol, (unsigned*)tail);
    BRCNN_LAUNCH_CHECK();
    hipLaunchKernelGGL(dx_ordered_shift_kernel, dim3(1), dim3(1), 0, s, tail, 62 - hb);
    BRCNN_LAUNCH_CHECK();
    if (dtype == BRCNN_DT_F32)
        hipLaunchKernelGGL((deform_col2im_nhwc_kernel<BRCNN_DT_F32, true>), grid, dim3(256), 0, s, x, offset_mask, dcol, acc,
                           d_offset_mask, batch, height, width, channels, Ho, Wo, kh, kw, stride, pad, dilation, om_stride,
                           channels_padded, deform_groups, modulated);
    else if (dtype == BRCNN_DT_F16)
        hipLaunchKernelGGL((deform_col2im_nhwc_kernel<BRCNN_DT_F16, true>), grid, dim3(256), 0, s, x, offset_mask, dcol, acc,
                           d_offset_mask, batch, height, width, channels, Ho, Wo, kh, kw, stride, pad, dilation, om_stride,
                           channels_padded, deform_groups, modulated);
    else
        hipLaunchKernelGGL((deform_col2im_nhwc_kernel<BRCNN_DT_BF16, true>), grid, dim3(256), 0, s, x, offset_mask, dcol, acc,
                           d_offset_mask, batch, height, width, channels, Ho, Wo, kh, kw, stride, pad, dilation, om_stride,
                           channels_padded, deform_groups, modulated);
    BRCNN_LAUNCH_CHECK();
    long long g = (n + 255) / 256;
    if (g > 8192) g = 8192;
    hipLaunchKernelGGL(dx_fixed_to_f32_kernel, dim3((unsigned)g), dim3(256), 0, s, (const long long*)workspace, dx, n);
    BRCNN_LAUNCH_CHECK();
    return 0;
}
