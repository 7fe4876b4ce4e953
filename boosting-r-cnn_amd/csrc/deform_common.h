// The sampled value of a deformable 3x3 conv (DCNv2, or DCN v1 = the mask factor identically 1) in the 16-bit modes, shared by the
// 16-bit im2col (deform.hip) and the fused conv (deform_conv_bf16.hip): the same fp32 arithmetic in the same order as
// deform_im2col_nhwc_kernel (the library is built with -ffp-contract=off, so neither form fuses a multiply-add the
// other does not), then ONE round to nearest even.  The fused kernel's A operand is therefore the 16-bit column matrix
// bit for bit, which is what makes it testable against an fp64 GEMM of those columns.
#pragma once
#include "common.h"

#if defined(__HIPCC__)
// one (output pixel, tap): four corner pixels (element offset of channel 0 inside the image, 0 where the corner is
// outside the map), which of them are inside (bits 0..3), the bilinear corner weights and sigmoid(mask logit).
// A tap whose sample point lies outside (-1, H) x (-1, W) gets no corners, zero weights and a zero mask.
// modulated = false (DCN v1): the mask factor is 1 and no sigmoid is evaluated (x * 1.f is exact, so the blend below is
// the v2 arithmetic with that factor).  With deform groups the caller passes the offsets / logit of the channels' group.
struct DeformTapGeom {
    int off1, off2, off3, off4;
    unsigned ok;
    float w1, w2, w3, w4;
    float mask;
};

// hb / wb: ho * stride - pad + i * dilation and its column counterpart (the integer base of the tap's sample point)
__device__ __forceinline__ DeformTapGeom deform_tap_geom(float off_h, float off_w, float mask_logit, int hb, int wb,
                                                         int H, int W, int C, bool pixel_ok, bool modulated = true) {
    DeformTapGeom g;
    const float mask = modulated ? 1.f / (1.f + expf(-mask_logit)) : 1.f;
    const float h_im = (float)hb + off_h;
    const float w_im = (float)wb + off_w;
    g.ok = 0u;
    g.mask = 0.f;
    g.off1 = g.off2 = g.off3 = g.off4 = 0;
    g.w1 = g.w2 = g.w3 = g.w4 = 0.f;
    if (pixel_ok && h_im > -1.f && w_im > -1.f && h_im < (float)H && w_im < (float)W) {
        const int h_low = (int)floorf(h_im), w_low = (int)floorf(w_im);
        const int h_high = h_low + 1, w_high = w_low + 1;
        const float lh = h_im - (float)h_low, lw = w_im - (float)w_low;
        const float hh = 1.f - lh, hw = 1.f - lw;
        g.w1 = hh * hw; g.w2 = hh * lw; g.w3 = lh * hw; g.w4 = lh * lw;
        g.mask = mask;
        const bool ok1 = h_low >= 0 && w_low >= 0, ok2 = h_low >= 0 && w_high <= W - 1;
        const bool ok3 = h_high <= H - 1 && w_low >= 0, ok4 = h_high <= H - 1 && w_high <= W - 1;
        g.ok = (ok1 ? 1u : 0u) | (ok2 ? 2u : 0u) | (ok3 ? 4u : 0u) | (ok4 ? 8u : 0u);
        g.off1 = ok1 ? (h_low * W + w_low) * C : 0;
        g.off2 = ok2 ? (h_low * W + w_high) * C : 0;
        g.off3 = ok3 ? (h_high * W + w_low) * C : 0;
        g.off4 = ok4 ? (h_high * W + w_high) * C : 0;
    }
    return g;
}

template <int DT> __device__ __forceinline__ float deform_e2f(unsigned short h) {
    return DT == BRCNN_DT_F16 ? brcnn_h2f(h) : brcnn_b2f(h);
}

// eight channels: the four corners' 16-byte loads (from the clamped offsets, loaded unconditionally) -> eight samples,
// rounded once to the 16-bit type and packed
template <int DT>
__device__ __forceinline__ uint4 deform_sample8(const DeformTapGeom& g, uint4 v1, uint4 v2, uint4 v3, uint4 v4) {
    // a corner outside the map reads +0 (its load came from the clamped address): the bit pattern masked to zero
    const unsigned k1 = (g.ok & 1u) ? ~0u : 0u, k2 = (g.ok & 2u) ? ~0u : 0u;
    const unsigned k3 = (g.ok & 4u) ? ~0u : 0u, k4 = (g.ok & 8u) ? ~0u : 0u;
    const unsigned r1[4] = {v1.x & k1, v1.y & k1, v1.z & k1, v1.w & k1}, r2[4] = {v2.x & k2, v2.y & k2, v2.z & k2, v2.w & k2};
    const unsigned r3[4] = {v3.x & k3, v3.y & k3, v3.z & k3, v3.w & k3}, r4[4] = {v4.x & k4, v4.y & k4, v4.z & k4, v4.w & k4};
    unsigned o[4];
#pragma unroll
    for (int d = 0; d < 4; d++) {
        float s[2];
#pragma unroll
        for (int e = 0; e < 2; e++) {
            const int sh = 16 * e;
            const float a1 = deform_e2f<DT>((unsigned short)(r1[d] >> sh)), a2 = deform_e2f<DT>((unsigned short)(r2[d] >> sh));
            const float a3 = deform_e2f<DT>((unsigned short)(r3[d] >> sh)), a4 = deform_e2f<DT>((unsigned short)(r4[d] >> sh));
            s[e] = (g.w1 * a1 + g.w2 * a2 + g.w3 * a3 + g.w4 * a4) * g.mask;
        }
        o[d] = DT == BRCNN_DT_F16 ? brcnn_pk2h(s[0], s[1]) : brcnn_pk2b(s[0], s[1]);
    }
    return make_uint4(o[0], o[1], o[2], o[3]);
}
#endif
