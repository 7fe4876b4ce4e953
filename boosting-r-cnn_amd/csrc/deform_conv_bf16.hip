// Fused deformable 3x3 conv (DCNv2 of the r2_101 recipes; DCN v1 / DCNv2 with deform groups of the ResNet dconv_c3-c5
// backbones) in the 16-bit modes:
//     y = act(scale * (sum_k col[m,k] * W[co,k]) + shift)
// in ONE launch, the column matrix never written to memory (the two-launch form writes (N*Ho*Wo, 9*Cp) columns and the
// GEMM reads them back: ~155 MB per stage-3 conv at batch 8 x 800 x 1344 in 16 bits).
//   x (N,H,W,Cp) bf16 / fp16, Cp % 64 == 0; offset_mask (N,Ho,Wo,om_stride >= 27) fp32, the raw conv_offset output (the
//   offsets are not rounded to 16 bits: at a coordinate of ~100 a bf16 offset is off by up to half a pixel);
//   w (Cout,3,3,Cp) in the K order (tap, c) of the columns; Cout % 64 == 0 (output-channel blocks in grid.y); y (N,Ho,Wo,Cout)
//   16-bit.  Deform groups G: (Cp / G) % 64 == 0, so every K step lies inside one group; the geometry is rebuilt at every
//   (tap, group) unit and its offsets are requested one unit ahead.  MOD = false (v1): no mask load, no sigmoid.
// A workgroup (4 waves, 2 x 2) computes 128 output pixels x BN = 64 * NB output channels on v_mfma_f32_32x32x16 with fp32
// accumulation; one K step = one tap x 64 channels.  Per step every thread gathers four 16-byte chunks (32 channels) of
// the four bilinear corners of one (pixel, tap), blends them in fp32 through deform_sample8 (deform_common.h: the 16-bit
// im2col's routine, so the A operand equals the 16-bit columns bit for bit), and writes the rounded A tile into swizzled
// LDS; the weight tile arrives beside it by LDS DMA.  The next step's corner loads (and weight DMA) are issued before the
// current step's MFMAs, so the gather runs under the matrix work; one barrier per step.  The tap geometry (corner
// offsets, bilinear weights x sigmoid(mask)) lives in registers for the Cp / 64 steps of a tap; the three fp32
// offset / mask values of the next tap are requested one tap ahead.
#include "common.h"
#include "deform_common.h"
#include "policy.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef __attribute__((address_space(3))) void* lds_ptr_t;
constexpr int BM = 128;
constexpr int A_BUF = BM * 128;          // bytes of one A buffer (128 rows of 64 elements)

struct DcnParams {
    const unsigned short* x;
    const float* om;
    const unsigned short* w;
    const float* scale;
    const float* shift;
    unsigned short* y;
    int H, W, Cp, Ho, Wo, M, stride, pad, om_stride, Cout, relu, tiles_m;
    int G, cbg;                     // deform groups, 64-channel blocks per group
    unsigned w_bytes;
};

// the three fp32 offset / mask values of one (tap, group) of a pixel's offset_mask row
template <bool MOD>
__device__ __forceinline__ void dcn_load_om(float (&om_n)[3], const float* omg, int tap, int grp, int G) {
    om_n[0] = omg[18 * grp + 2 * tap];
    om_n[1] = omg[18 * grp + 2 * tap + 1];
    om_n[2] = MOD ? omg[18 * G + 9 * grp + tap] : 0.f;
}

// the four corners x four 16-byte chunks of one step (clamped offsets: every load is issued)
__device__ __forceinline__ void dcn_load_corners(uint4 (&cv)[4][4], const DeformTapGeom& g, const unsigned short* xg, int cb) {
    const unsigned short* x1 = xg + g.off1 + cb * 64;
    const unsigned short* x2 = xg + g.off2 + cb * 64;
    const unsigned short* x3 = xg + g.off3 + cb * 64;
    const unsigned short* x4 = xg + g.off4 + cb * 64;
#pragma unroll
    for (int c = 0; c < 4; c++) {
        cv[0][c] = *reinterpret_cast<const uint4*>(x1 + c * 8);
        cv[1][c] = *reinterpret_cast<const uint4*>(x2 + c * 8);
        cv[2][c] = *reinterpret_cast<const uint4*>(x3 + c * 8);
        cv[3][c] = *reinterpret_cast<const uint4*>(x4 + c * 8);
    }
}

// the four blended, rounded chunks of a thread into its A row (logical chunk 4 gh + c at physical (4 gh + c) ^ sw)
template <int DT>
__device__ __forceinline__ void dcn_store_a(unsigned char* a_row, const DeformTapGeom& g, const uint4 (&cv)[4][4], int gh, int sw) {
#pragma unroll
    for (int c = 0; c < 4; c++)
        *reinterpret_cast<uint4*>(a_row + (((4 * gh + c) ^ sw) * 16)) = deform_sample8<DT>(g, cv[0][c], cv[1][c], cv[2][c], cv[3][c]);
}

// the weight tile of step s (BN rows x 64 channels of one tap) into the B buffer at `dst`, by LDS DMA
template <int NB>
__device__ __forceinline__ void dcn_dma_w(const unsigned short* w, unsigned w_bytes, unsigned char* dst, const int* b_off,
                                          int wave, int s, int CB, int Cp) {
    const __amdgpu_buffer_rsrc_t rsrc_w = __builtin_amdgcn_make_buffer_rsrc((void*)w, 0, (int)w_bytes, 0x00020000);
    const int tap = s / CB, cb = s - tap * CB;
    const int k_off = (tap * Cp + cb * 64) * 2;
#pragma unroll
    for (int j = 0; j < 2 * NB; j++)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_w, (lds_ptr_t)(dst + (wave * 2 * NB + j) * 1024), 16, b_off[j] + k_off, 0, 0, 0);
}

template <int DT, int NB, bool MOD>     // NB: 32-channel MFMA tiles per wave; the workgroup covers BN = 64 * NB output channels
__global__ __launch_bounds__(256, 2) void deform_conv16_kernel(DcnParams p) {
    constexpr int BN = 64 * NB, B_BUF = BN * 128;
    // LDS: A buffers [0, 32K), B buffers [32K, 32K + 2 * B_BUF); step s uses buffers s & 1
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* As = smem;
    unsigned char* Bs = smem + 2 * A_BUF;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;     // a wave: 64 pixel rows (two 32-row tiles) x BN / 2 channels
    const int li = lane & 31, lh = lane >> 5;

    int tile_m;
    {   // consecutive tiles on one XCD (their halo rows meet in one L2)
        const int nwg = p.tiles_m, q = nwg >> 3, r = nwg & 7, xcd = blockIdx.x & 7, loc = blockIdx.x >> 3;
        tile_m = ((xcd < r) ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + loc;
    }
    const int m0 = tile_m * BM;
    const int co0 = blockIdx.y * BN;
    const int CB = p.Cp >> 6, S = 9 * CB;        // 64-channel blocks per tap, K steps

    // ---- gather assignment: thread -> pixel row gr of the tile, 16-byte chunks 4 gh .. 4 gh + 3 of the 64-channel row
    const int gr = tid >> 1, gh = tid & 1;
    const int gm = m0 + gr;
    const bool gvalid = gm < p.M;
    const int gmc = gvalid ? gm : 0;
    const int HoWo = p.Ho * p.Wo;
    const int gn = gmc / HoWo;
    const int grem = gmc - gn * HoWo;
    const int gho = grem / p.Wo, gwo = grem - gho * p.Wo;
    const int hb0 = gho * p.stride - p.pad, wb0 = gwo * p.stride - p.pad;
    const unsigned short* xg = p.x + (size_t)gn * p.H * p.W * p.Cp + gh * 32;
    const float* omg = p.om + (size_t)gmc * p.om_stride;
    unsigned char* a_dst = As + gr * 128;
    const int a_sw = (gr >> 1) & 7;

    // ---- weight DMA: 8-row groups (lane: row rg of the group, physical chunk pc, logical chunk pc ^ ((row >> 1) & 7));
    // BN / 8 groups, NB * 2 per wave
    const int rg = lane >> 3, pc = lane & 7;
    int b_off[2 * NB];
#pragma unroll
    for (int j = 0; j < 2 * NB; j++) {
        const int r = (wave * 2 * NB + j) * 8 + rg;
        b_off[j] = ((co0 + r) * 9 * p.Cp + (pc ^ ((r >> 1) & 7)) * 8) * 2;
    }

    // ---- tap geometry (registers) and the corner loads of one step
    DeformTapGeom g;
    float om_n[3];                  // offset / mask logit of the next tap, requested one tap ahead
    uint4 cv[4][4];                 // [corner][chunk]

    // ---- fragment reads (row R = base + li, logical chunk 2 kk + lh at physical chunk c ^ ((R >> 1) & 7)); the second
    // 32-row tile of a wave (and the second 32-channel tile of B) lies 4096 bytes further
    const int sw = (li >> 1) & 7;
    unsigned chb[4];
#pragma unroll
    for (int kk = 0; kk < 4; kk++) chb[kk] = (unsigned)(((2 * kk + lh) ^ sw) * 16);
    const unsigned a_lane = (unsigned)(size_t)(lds_ptr_t)(As + (wm * 64 + li) * 128);
    const unsigned b_lane = (unsigned)(size_t)(lds_ptr_t)(Bs + (wn * 32 * NB + li) * 128);
    f32x4 av[2][2], bv[2][NB];
    auto frag_read = [&](int slot, unsigned a_addr, unsigned b_addr) {
        asm volatile("ds_read_b128 %0, %1" : "=v"(av[slot][0]) : "v"(a_addr) : "memory");
        asm volatile("ds_read_b128 %0, %1 offset:4096" : "=v"(av[slot][1]) : "v"(a_addr) : "memory");
        asm volatile("ds_read_b128 %0, %1" : "=v"(bv[slot][0]) : "v"(b_addr) : "memory");
        if constexpr (NB == 2) asm volatile("ds_read_b128 %0, %1 offset:4096" : "=v"(bv[slot][NB - 1]) : "v"(b_addr) : "memory");
    };
    auto frag_wait = [&](int slot) {
        if constexpr (NB == 2)
            asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(av[slot][0]), "+v"(av[slot][1]), "+v"(bv[slot][0]), "+v"(bv[slot][NB - 1]) :: "memory");
        else
            asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(av[slot][0]), "+v"(av[slot][1]), "+v"(bv[slot][0]) :: "memory");
    };
    auto mma = [&](f32x16& c, const f32x4& b, const f32x4& a) {
        if constexpr (DT == BRCNN_DT_F16)
            c = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, b), __builtin_bit_cast(f16x8, a), c, 0, 0, 0);
        else
            c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, b), __builtin_bit_cast(bf16x8, a), c, 0, 0, 0);
    };

    f32x16 acc[2][NB];
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int b = 0; b < NB; b++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[a][b][r] = 0.f;

    // prologue: the geometry of unit 0 = (tap 0, group 0), step 0's corners and weights, unit 1's offsets
    // (unit u = tap * G + group, in the order the K loop meets them)
    const int G = p.G, cbg = p.cbg;
    dcn_load_om<MOD>(om_n, omg, 0, 0, G);
    g = deform_tap_geom(om_n[0], om_n[1], om_n[2], hb0, wb0, p.H, p.W, p.Cp, gvalid, MOD);
    dcn_load_corners(cv, g, xg, 0);
    dcn_dma_w<NB>(p.w, p.w_bytes, Bs, b_off, wave, 0, CB, p.Cp);
    dcn_load_om<MOD>(om_n, omg, G > 1 ? 0 : 1, G > 1 ? 1 : 0, G);

    for (int s = 0; s < S; s++) {
        const int cur = s & 1;
        // step s's corners, weights and the next tap's offsets have landed; the A tile of step s goes into buffer cur,
        // which the MFMAs of step s - 2 were the last to read (every wave passed the barrier of step s - 1 after them)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        dcn_store_a<DT>(a_dst + cur * A_BUF, g, cv, gh, a_sw);
        __syncthreads();
        if (s + 1 < S) {
            const int tap = (s + 1) / CB, cb = (s + 1) - tap * CB;
            const int grp = cb / cbg;
            if (cb - grp * cbg == 0) {      // the channel chunk enters the next group (or tap): its geometry, and the next unit's offsets
                const int ti = tap / 3, tj = tap - ti * 3;
                g = deform_tap_geom(om_n[0], om_n[1], om_n[2], hb0 + ti, wb0 + tj, p.H, p.W, p.Cp, gvalid, MOD);
                const int un = tap * G + grp + 1;
                if (un < 9 * G) {
                    const int tn = un / G;
                    dcn_load_om<MOD>(om_n, omg, tn, un - tn * G, G);
                }
            }
            dcn_load_corners(cv, g, xg, cb);
            dcn_dma_w<NB>(p.w, p.w_bytes, Bs + (cur ^ 1) * B_BUF, b_off, wave, s + 1, CB, p.Cp);
        }
        const unsigned a_cur = a_lane + cur * A_BUF, b_cur = b_lane + cur * B_BUF;
        frag_read(0, a_cur + chb[0], b_cur + chb[0]);
        frag_wait(0);
#pragma unroll
        for (int kk = 0; kk < 4; kk++) {
            const int sl = kk & 1;
            if (kk + 1 < 4) frag_read(sl ^ 1, a_cur + chb[kk + 1], b_cur + chb[kk + 1]);
#pragma unroll
            for (int nb = 0; nb < NB; nb++) {
                mma(acc[0][nb], bv[sl][nb], av[sl][0]);
                mma(acc[1][nb], bv[sl][nb], av[sl][1]);
            }
            if (kk + 1 < 4) frag_wait(sl ^ 1);
        }
    }

    // ---- epilogue (D^T = W A^T: lane l holds pixel row l & 31 of its tile and, per register group g, the four channels
    // 8 g + 4 (l >> 5) + (0..3) of its 32-channel tile): y = act(acc * scale + shift), one rounding
#pragma unroll
    for (int nb = 0; nb < NB; nb++) {
#pragma unroll
        for (int gq = 0; gq < 4; gq++) {
            const int ch = co0 + wn * 32 * NB + nb * 32 + 8 * gq + 4 * lh;
            float sc[4], sh[4];
#pragma unroll
            for (int e = 0; e < 4; e++) { sc[e] = p.scale ? p.scale[ch + e] : 1.f; sh[e] = p.shift ? p.shift[ch + e] : 0.f; }
#pragma unroll
            for (int tm = 0; tm < 2; tm++) {
                const int m = m0 + wm * 64 + tm * 32 + li;
                float v[4];
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    float t = acc[tm][nb][4 * gq + e];
                    if (p.scale) t = t * sc[e] + sh[e];
                    else if (p.shift) t = t + sh[e];
                    v[e] = p.relu ? fmaxf(t, 0.f) : t;
                }
                uint2 o;
                o.x = DT == BRCNN_DT_F16 ? brcnn_pk2h(v[0], v[1]) : brcnn_pk2b(v[0], v[1]);
                o.y = DT == BRCNN_DT_F16 ? brcnn_pk2h(v[2], v[3]) : brcnn_pk2b(v[2], v[3]);
                if (m < p.M) *reinterpret_cast<uint2*>(p.y + (size_t)m * p.Cout + ch) = o;
            }
        }
    }
}

template <int DT, int NB, bool MOD>
int launch_dcn16(const DcnParams& p, hipStream_t s) {
    const size_t lds = (size_t)2 * A_BUF + 2 * (64 * NB) * 128;
    hipLaunchKernelGGL((deform_conv16_kernel<DT, NB, MOD>), dim3(p.tiles_m, p.Cout / (64 * NB)), dim3(256), lds, s, p);
    BRCNN_LAUNCH_CHECK();
    brcnn::count(brcnn::g_counters.dcn_fused_launches);
    return 0;
}

// what the fused kernel takes: 64-channel K steps inside one deform group, whole 64-channel output blocks
bool dcn16_shape_ok(int channels, int cout, int stride, int pad, int groups, int dtype) {
    return channels > 0 && !(channels & 63) && groups > 0 && !(channels % groups) && !((channels / groups) & 63) && cout > 0 &&
           !(cout & 63) && (stride == 1 || stride == 2) && pad >= 0 && pad <= 2 && (dtype == BRCNN_DT_BF16 || dtype == BRCNN_DT_F16);
}

int dcn16_run(const void* x, const float* offset_mask, const void* w, const float* scale, const float* shift, void* y,
              int batch, int height, int width, int channels, int cout, int stride, int pad, int relu, int om_stride,
              int groups, int modulated, int dtype, void* stream) {
    // (a padded map smaller than the kernel has no output: C's truncating division would give it one row)
    if (height + 2 * pad < 3 || width + 2 * pad < 3) return BRCNN_EINVAL;
    const int Ho = (height + 2 * pad - 3) / stride + 1, Wo = (width + 2 * pad - 3) / stride + 1;
    const long long M = (long long)batch * Ho * Wo;
    // every element offset (x, y, the weights' byte range of the buffer descriptor) fits 32 bits
    if ((long long)batch * height * width * channels >= 0x7fffffffLL || M * cout >= 0x7fffffffLL ||
        M * om_stride >= 0x7fffffffLL || (long long)cout * 9 * channels * 2 >= 0x7fffffffLL)
        return BRCNN_EINVAL;
    DcnParams p;
    p.x = (const unsigned short*)x; p.om = offset_mask; p.w = (const unsigned short*)w; p.scale = scale; p.shift = shift;
    p.y = (unsigned short*)y;
    p.H = height; p.W = width; p.Cp = channels; p.Ho = Ho; p.Wo = Wo; p.M = (int)M; p.stride = stride; p.pad = pad;
    p.om_stride = om_stride; p.Cout = cout; p.relu = relu ? 1 : 0; p.tiles_m = (int)((M + BM - 1) / BM);
    p.w_bytes = (unsigned)((long long)cout * 9 * channels * 2);
    p.G = groups; p.cbg = (channels >> 6) / groups;
    hipStream_t s = (hipStream_t)stream;
    // 128-channel workgroups wherever Cout is a multiple of 128: one gather per two 64-channel slices.  (64-channel workgroups
    // on the short stage-4 maps -- twice the workgroups, each gathering its own A tiles -- measured slower: the gather is the bound)
    const bool wide = !(cout & 127);
    if (modulated) {
        if (dtype == BRCNN_DT_F16) return wide ? launch_dcn16<BRCNN_DT_F16, 2, true>(p, s) : launch_dcn16<BRCNN_DT_F16, 1, true>(p, s);
        return wide ? launch_dcn16<BRCNN_DT_BF16, 2, true>(p, s) : launch_dcn16<BRCNN_DT_BF16, 1, true>(p, s);
    }
    if (dtype == BRCNN_DT_F16) return wide ? launch_dcn16<BRCNN_DT_F16, 2, false>(p, s) : launch_dcn16<BRCNN_DT_F16, 1, false>(p, s);
    return wide ? launch_dcn16<BRCNN_DT_BF16, 2, false>(p, s) : launch_dcn16<BRCNN_DT_BF16, 1, false>(p, s);
}

}  // namespace

BRCNN_API int brcnn_deform_conv_nhwc(const void* x, const float* offset_mask, const void* w, const float* scale,
                                     const float* shift, void* y, int batch, int height, int width, int channels,
                                     int cout, int stride, int pad, int relu, int om_stride, int dtype, void* stream) {
    if (!x || !offset_mask || !w || !y || batch <= 0 || height <= 0 || width <= 0 || channels <= 0 || (channels & 63) ||
        (cout != 64 && cout != 128 && cout != 256) || (stride != 1 && stride != 2) || pad < 0 || pad > 2 ||
        om_stride < 27 || (dtype != BRCNN_DT_BF16 && dtype != BRCNN_DT_F16))
        return BRCNN_EINVAL;
    return dcn16_run(x, offset_mask, w, scale, shift, y, batch, height, width, channels, cout, stride, pad, relu, om_stride, 1, 1,
                     dtype, stream);
}

// deform groups, the unmodulated form (DCN v1: offset rows of 18 * deform_groups floats, no mask) and any cout % 64 == 0.
// Refuses (BRCNN_EINVAL) what the kernel does not take -- (channels / deform_groups) % 64 != 0 above all: the caller then
// runs brcnn_deform_im2col_nhwc_g + the GEMM (brcnn_deform_conv_route answers beforehand).
BRCNN_API int brcnn_deform_conv_nhwc_g(const void* x, const float* offset_mask, const void* w, const float* scale,
                                       const float* shift, void* y, int batch, int height, int width, int channels,
                                       int cout, int stride, int pad, int relu, int om_stride, int deform_groups,
                                       int modulated, int dtype, void* stream) {
    if (!x || !offset_mask || !w || !y || batch <= 0 || height <= 0 || width <= 0 || (modulated != 0 && modulated != 1) ||
        !dcn16_shape_ok(channels, cout, stride, pad, deform_groups, dtype) ||
        om_stride < (modulated ? 27 : 18) * (long long)deform_groups)
        return BRCNN_EINVAL;
    return dcn16_run(x, offset_mask, w, scale, shift, y, batch, height, width, channels, cout, stride, pad, relu, om_stride,
                     deform_groups, modulated, dtype, stream);
}

// 1: the 16-bit deformable conv of this shape runs on the fused kernel, 0: as im2col + GEMM.  policy dcn_fused
// (brcnn_conv_set_tile(-13, n)): 0 never fused, 2 wherever brcnn_deform_conv_nhwc_g accepts the shape, 1 (default) the
// rule measured on the ResNet c3-c5 and Res2Net shapes (profiles/resnet_dcn_bench_*.txt).
BRCNN_API int brcnn_deform_conv_route(int batch, int height, int width, int channels, int cout, int stride, int pad,
                                      int deform_groups, int dtype) {
    if (batch <= 0 || height <= 0 || width <= 0 || !dcn16_shape_ok(channels, cout, stride, pad, deform_groups, dtype)) return 0;
    if (brcnn::g_policy.dcn_fused != 1) return brcnn::g_policy.dcn_fused == 2;
    // The measured rule (profiles/resnet_dcn_bench_*.txt, res2net16_deform_bench_*.txt): a workgroup column covers at most 128
    // output channels, and every column gathers and blends the A tiles again.  With one column (cout <= 128) the fused
    // kernel took 0.6-0.9 of the time of im2col + GEMM on every shape measured; with two or four columns (cout 256 / 512:
    // the gather done two / four times) 1.3-2.2 of it.
    return cout <= 128;
}
