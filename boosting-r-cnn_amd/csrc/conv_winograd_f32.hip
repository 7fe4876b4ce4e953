// fp32 Winograd F(2x2, 3x3) convolution (3x3, stride 1, pad 1) over the segment table of brcnn_conv2d_nhwc_multi: 16
// multiplies serve a 2x2 output tile, 4 per output and input channel instead of 9 -- the RPN tower's 256 -> 256 layers
// are MFMA-bound at 0.88 of the fp32 roof, so the remaining lever is fewer MFMAs.  Three kernels:
//   filter     U[xi][co][ci] = (G g G^T)[xi], xi = 4 i + j, once per weight (brcnn_winograd_filter_f32)
//   input      V[xi][tile][ci] = (B^T d B)[xi] of the 4x4 patch of each 2x2 output tile; optionally d <- relu?(gn(d)) with
//              the finalized (mean, rstd) of brcnn_groupnorm_nhwc_multi in gn_apply_rows_kernel's expression (misc.hip) --
//              the operand is then bit for bit the transform of what that kernel would have written; the halo is zero
//              AFTER the prologue (the conv pads the normalised tensor)
//   gemm       per workgroup 64 tiles x 128 channels (the tower; 32 x 128 and 64 x 64 for the single-layer entry, see
//              wino_gemm_kernel): for each xi a K = Cin product into one temporary accumulator set
//              (v_mfma_f32_32x32x2_f32, LDS-DMA staging of step s + 1 under the MFMAs of step s, the 16 x Cin / 32 steps
//              run as ONE pipelined loop), then tmp is added / subtracted into y00 y01 y10 y11 by A^T M A (per-lane VALU:
//              the 16 products share one lane mapping); read-out with scale / shift / ReLU to the pixels of each
//              tile that lie inside the map.
// Tiles are counted per segment as ceil(H / 2) ceil(W / 2) per image.  A launch pair may cover a CHUNK of the tiles
// [tile0, tile0 + nt) so that V of a chunk stays in the Infinity Cache between the two kernels: measured slower at every
// split of the tower (profiles/f32_winograd.txt), so one pair per call is the default (policy.h: f32_winograd_chunks).
#include "conv_common.h"
#include "policy.h"

namespace {
using namespace brcnn_conv;

typedef __attribute__((address_space(3))) void* lds_ptr_t;

struct WinoSegs {
    int nseg, batch;
    int H[BRCNN_MAX_LEVELS], W[BRCNN_MAX_LEVELS], TH[BRCNN_MAX_LEVELS], TW[BRCNN_MAX_LEVELS];
    int t0[BRCNN_MAX_LEVELS + 1];       // first tile of segment s (t0[nseg ..] = all tiles)
    int r0[BRCNN_MAX_LEVELS + 1];       // first pixel row of segment s in the concatenated (rows, C)
};

// tile -> (segment, pixel row of its top-left output pixel (2 th, 2 tw), rows / columns of the tile inside the map)
struct WinoTile { int seg, n, h, w; };
__device__ __forceinline__ WinoTile wino_tile(const WinoSegs& sg, int t) {
    int s = 0;
#pragma unroll
    for (int i = 1; i < BRCNN_MAX_LEVELS; i++)
        if (i < sg.nseg && t >= sg.t0[i]) s = i;
    const int l = t - sg.t0[s];
    const int per = sg.TH[s] * sg.TW[s];
    const int n = l / per, rem = l - n * per;
    const int th = rem / sg.TW[s];
    return {s, n, 2 * th, 2 * (rem - th * sg.TW[s])};
}

// ---- filter transform: one thread per (co, ci); G = [1 0 0; .5 .5 .5; .5 -.5 .5; 0 0 1]
__global__ __launch_bounds__(256) void wino_filter_kernel(const float* __restrict__ w, float* __restrict__ u, int Cout, int Cin) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= Cout * Cin) return;
    const int co = idx / Cin, ci = idx - co * Cin;
    float g[3][3], t[4][3];
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
        for (int b = 0; b < 3; b++) g[a][b] = w[((size_t)(co * 3 + a) * 3 + b) * Cin + ci];
#pragma unroll
    for (int b = 0; b < 3; b++) {
        t[0][b] = g[0][b];
        t[1][b] = 0.5f * (g[0][b] + g[1][b] + g[2][b]);
        t[2][b] = 0.5f * (g[0][b] - g[1][b] + g[2][b]);
        t[3][b] = g[2][b];
    }
#pragma unroll
    for (int a = 0; a < 4; a++) {
        const float o[4] = {t[a][0], 0.5f * (t[a][0] + t[a][1] + t[a][2]), 0.5f * (t[a][0] - t[a][1] + t[a][2]), t[a][2]};
#pragma unroll
        for (int b = 0; b < 4; b++) u[((size_t)(a * 4 + b) * Cout + co) * Cin + ci] = o[b];
    }
}

// ---- input transform: one thread per (tile, 4 channels); B^T = [1 0 -1 0; 0 1 1 0; 0 -1 1 0; 0 1 0 -1]
__global__ __launch_bounds__(256) void wino_input_kernel(const float* __restrict__ x, float* __restrict__ v, WinoSegs sg,
                                                        int tile0, int nt, int C, const double* __restrict__ stats,
                                                        const float* __restrict__ gamma, const float* __restrict__ beta,
                                                        int G, int relu_in) {
    const int cq = C >> 2;
    const unsigned idx = blockIdx.x * 256u + threadIdx.x;
    if (idx >= (unsigned)nt * (unsigned)cq) return;
    const int tl = (int)(idx / (unsigned)cq), c0 = ((int)idx - tl * cq) * 4;
    const WinoTile t = wino_tile(sg, tile0 + tl);
    const int H = sg.H[t.seg], W = sg.W[t.seg];
    const float* xs = x + ((size_t)sg.r0[t.seg] + (size_t)t.n * H * W) * C + c0;
    float mean[4], rstd[4], gm[4], bt[4];
    if (stats) {
        const int cpg = C / G;
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const int c = c0 + e;
            const float2 mr = reinterpret_cast<const float2*>(stats + ((size_t)(t.seg * sg.batch + t.n) * G + c / cpg) * 2)[0];
            mean[e] = mr.x; rstd[e] = mr.y; gm[e] = gamma[c]; bt[e] = beta[c];
        }
    }
    float d[4][4][4];
#pragma unroll
    for (int a = 0; a < 4; a++)
#pragma unroll
        for (int b = 0; b < 4; b++) {
            const int h = t.h - 1 + a, w = t.w - 1 + b;
            const bool ok = (unsigned)h < (unsigned)H && (unsigned)w < (unsigned)W;
            float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
            if (ok) q = *reinterpret_cast<const float4*>(xs + ((size_t)h * W + w) * C);
            float in[4] = {q.x, q.y, q.z, q.w};
            if (stats) {
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    // gn_apply_rows_kernel's expression and order; the halo stays zero: the conv pads the normalised tensor
                    const float o = (in[e] - mean[e]) * rstd[e] * gm[e] + bt[e];
                    in[e] = ok ? (relu_in ? fmaxf(o, 0.f) : o) : 0.f;
                }
            }
#pragma unroll
            for (int e = 0; e < 4; e++) d[a][b][e] = in[e];
        }
    float* vs = v + (size_t)tl * C + c0;
    const size_t xi_stride = (size_t)nt * C;
#pragma unroll
    for (int e = 0; e < 4; e++) {
        float r[4][4];
#pragma unroll
        for (int b = 0; b < 4; b++) {
            r[0][b] = d[0][b][e] - d[2][b][e];
            r[1][b] = d[1][b][e] + d[2][b][e];
            r[2][b] = d[2][b][e] - d[1][b][e];
            r[3][b] = d[1][b][e] - d[3][b][e];
        }
#pragma unroll
        for (int a = 0; a < 4; a++) {
            d[a][0][e] = r[a][0] - r[a][2];
            d[a][1][e] = r[a][1] + r[a][2];
            d[a][2][e] = r[a][2] - r[a][1];
            d[a][3][e] = r[a][1] - r[a][3];
        }
    }
#pragma unroll
    for (int a = 0; a < 4; a++)
#pragma unroll
        for (int b = 0; b < 4; b++)
            *reinterpret_cast<float4*>(vs + (size_t)(a * 4 + b) * xi_stride) = make_float4(d[a][b][0], d[a][b][1], d[a][b][2], d[a][b][3]);
}

// ---- GEMM + output transform
struct WinoGemmParams {
    const float* v;         // [16][nt][Cin]
    const float* u;         // [16][Cout][Cin]
    const float* scale;
    const float* shift;
    float* y;               // (rows, Cout)
    unsigned v_bytes, u_bytes;
    int tile0, nt, Cin, Cout, relu;
    int tiles_m, tiles_n;
    WinoSegs sg;
    // persistent launch (wino_gemm_kernel<.., true>; appended: the plain kernels read what they read before): the range table
    // [sk_wgs x (first item, count, 0, 0) | items (workgroup tile, first xi, end xi, hand-over slot)] of sk_plan_ranges, the
    // stream's hand-over slots (the four y accumulator sets of one workgroup tile each) and flags, the launch's epoch, the
    // host-mapped error word and the poll bound of a tail that waits for its head
    const int4* sk_items;
    float* sk_ws;
    unsigned* sk_flags;
    unsigned sk_epoch;
    unsigned* sk_err;
    int sk_spin_limit;
};

// Workgroup tile variants (WBM tiles x WBN output channels, four waves as WMW x WNW, a wave owns 32 x 32 NB):
//   1  64 x 128, 2 x 2 waves of 32 x 64: the tower's (the only one until the single-layer route; its code is unchanged)
//   2  32 x 128, four waves side by side, 32 x 32 each
//   3  64 x 64, 2 x 2 waves of 32 x 32
// The 32 x 32 wave tiles double the waves of a launch: the layers of 2 184 .. 8 400 tiles leave most CUs with ONE 64 x 128
// workgroup.  Every variant sums the K loop of an output in the same order, so the results are equal bit for bit.
constexpr int WBM_MAX = 64;             // launch chunks are whole row blocks of every variant

// A^T = [1 1 1 0; 0 1 -1 -1]: coefficient of M[i][j] (xi = 4 i + j) in y[a][b] is AT[a][i] AT[b][j]
__device__ __forceinline__ constexpr int wino_at(int a, int i) { return a == 0 ? (i < 3 ? 1 : 0) : (i == 0 ? 0 : (i == 1 ? 1 : -1)); }

// One work item: xi planes [xb, xe) of workgroup tile `tile` (the 16 x Cin / 32 steps of a tile are cut on xi boundaries
// only, so tmp is never handed over).  The plain launch runs one item per workgroup, all 16 planes of its tile (PERS = false:
// xb = 0, xe = 16 fold away and the code is the one-tile kernel's).  The persistent launch (PERS = true, wino_gemm_kernel)
// hands a workgroup a list of items: an item that stops short of xi = 16 stores its four y accumulator sets to
// sk_ws[slot] and publishes sk_flags[slot] = sk_epoch instead of reading out; an item that starts past xi = 0 waits for
// that flag (bounded poll, conv_igemm.hip's) and continues from those accumulators.  Every output sees its 16 products,
// each the same MFMA chain over Cin, folded into y in the order xi = 0 .. 15 either way: the two forms give the same bits.
// RING: stages of the LDS ring.  2 is the loop as it was: the DMA of step s + 1 is issued under the MFMAs of step s and drained
// (vmcnt(0)) before the barrier that ends the step.  3 keeps TWO steps in flight: step s waits only until its own operands
// have landed (counted vmcnt: the AG + BG loads of step s + 1 may still be out), takes the barrier, issues step s + 2 into
// the stage that step s - 1 has just left, and runs the same fragment reads and MFMAs in the same order.
// (the body exists in the device pass only: the host pass would instantiate the inline assembly, whose operand types depend on
// the template's parameters, against the host's constraints and drop the launch stub)
template <int WBM, int WBN, int WNW, bool PERS, int RING>
__device__ __forceinline__ void wino_gemm_item(const WinoGemmParams& p, float* smem, const int tile, const int xb_, const int xe_,
                                               const int slot) {
#if defined(__HIP_DEVICE_COMPILE__)
    constexpr int NB = WBN / (32 * WNW);        // 32-column blocks of a wave
    const int xb = PERS ? xb_ : 0, xe = PERS ? xe_ : 16;
    float* As = smem;
    float* Bs = smem + RING * WBM * 32;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WNW, wn = wave % WNW;
    const int li = lane & 31, lh = lane >> 5;

    const int tile_m = tile / p.tiles_n, tile_n = tile - tile_m * p.tiles_n;
    const int m0 = tile_m * WBM, n0 = tile_n * WBN;

    const __amdgpu_buffer_rsrc_t rsrc_v = __builtin_amdgcn_make_buffer_rsrc((void*)p.v, 0, (int)p.v_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsrc_u = __builtin_amdgcn_make_buffer_rsrc((void*)p.u, 0, (int)p.u_bytes, 0x00020000);

    // ---- DMA assignment (conv_igemm_f32_dma_kernel's): a wave moves 8-row groups, lane -> (row in group, physical chunk)
    constexpr int AG = WBM / 8 / 4, BG = WBN / 8 / 4;       // 64 x 128: 2, 4
    const int rg = lane >> 3, pc = lane & 7;
    int a_off[AG], b_off[BG];
#pragma unroll
    for (int j = 0; j < AG; j++) {
        const int r = (wave * AG + j) * 8 + rg;
        const int t = m0 + r;
        a_off[j] = t < p.nt ? (t * p.Cin + (pc ^ ((r >> 1) & 7)) * 4) * 4 : -1;
    }
#pragma unroll
    for (int j = 0; j < BG; j++) {
        const int r = (wave * BG + j) * 8 + rg;
        const int co = n0 + r;
        b_off[j] = co < p.Cout ? (co * p.Cin + (pc ^ ((r >> 1) & 7)) * 4) * 4 : -1;
    }
    const int nk = p.Cin / 32;
    const int a_xi = p.nt * p.Cin * 4, b_xi = p.Cout * p.Cin * 4;      // bytes between two xi planes (< 2^31 / 16: the host checks)
    int s_xi = xb, s_kc = 0;            // (xi, K chunk) of the step staged next
    auto dma_step = [&](int buf) {
        const int ao = s_xi * a_xi + s_kc * 128, bo = s_xi * b_xi + s_kc * 128;
        if (++s_kc == nk) { s_kc = 0; s_xi++; }
#pragma unroll
        for (int j = 0; j < AG; j++) {
            float* dst = As + buf * WBM * 32 + (wave * AG + j) * 8 * 32;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_v, (lds_ptr_t)dst, 16, a_off[j] >= 0 ? a_off[j] + ao : OOB, 0, 0, 0);
        }
#pragma unroll
        for (int j = 0; j < BG; j++) {
            float* dst = Bs + buf * WBN * 32 + (wave * BG + j) * 8 * 32;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_u, (lds_ptr_t)dst, 16, b_off[j] >= 0 ? b_off[j] + bo : OOB, 0, 0, 0);
        }
    };

    // ---- fragment reads (inline asm: a compiler-visible LDS read after an LDS-DMA would draw a vmcnt(0) in front of it,
    // conv_igemm.hip): row base + li, logical chunk 2 kk + lh at physical chunk ^ ((li >> 1) & 7)
    const int sw = (li >> 1) & 7;
    unsigned chb[4];
#pragma unroll
    for (int kk = 0; kk < 4; kk++) chb[kk] = (unsigned)(((2 * kk + lh) ^ sw) * 16);
    const unsigned a_lane = (unsigned)(size_t)(lds_ptr_t)(As + (wm * 32 + li) * 32);
    const unsigned b_lane = (unsigned)(size_t)(lds_ptr_t)(Bs + (wn * 32 * NB + li) * 32);
    f32x4 av[2], bv[2][NB];
    auto frag_read = [&](int slot, unsigned a_addr, unsigned b_addr) {
        asm volatile("ds_read_b128 %0, %1" : "=v"(av[slot]) : "v"(a_addr) : "memory");
        asm volatile("ds_read_b128 %0, %1" : "=v"(bv[slot][0]) : "v"(b_addr) : "memory");
        if constexpr (NB == 2) asm volatile("ds_read_b128 %0, %1 offset:4096" : "=v"(bv[slot][NB - 1]) : "v"(b_addr) : "memory");
    };
    auto frag_wait = [&](int slot) {
        if constexpr (NB == 2)
            asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(av[slot]), "+v"(bv[slot][0]), "+v"(bv[slot][NB - 1]) :: "memory");
        else
            asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(av[slot]), "+v"(bv[slot][0]) :: "memory");
    };

    f32x16 yacc[4][NB], tmp[NB];        // y00 y01 y10 y11 and the product of the current xi, NB 32-column blocks each
#pragma unroll
    for (int q = 0; q < 4; q++)
#pragma unroll
        for (int b = 0; b < NB; b++)
#pragma unroll
            for (int r = 0; r < 16; r++) yacc[q][b][r] = 0.f;

    dma_step(0);
    if constexpr (RING == 3) {
        if ((xe - xb) * nk > 1) dma_step(1);
    }
    if constexpr (PERS) {
        if (xb > 0) {
            // the planes below xb of this tile, published by the workgroup of the range below as its FIRST item: one lane
            // polls (bounded), one agent-scope acquire, then plain loads into the accumulators in their register layout
            // (the DMA above stays in flight under them)
            if (tid == 0) {
                int spins = 0;
                while (__hip_atomic_load(p.sk_flags + slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != p.sk_epoch &&
                       ++spins < p.sk_spin_limit)
                    __builtin_amdgcn_s_sleep(4);
                // a hand-over that never arrives must not end as a silent wrong result: the host-mapped error word
                // makes the next launch on any stream (and brcnn_conv_handover_status) return BRCNN_EHANDOVER
                if (spins >= p.sk_spin_limit)
                    __hip_atomic_store(p.sk_err, p.sk_epoch | 0x80000000u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            }
            __syncthreads();
            const f32x4* src = reinterpret_cast<const f32x4*>(p.sk_ws) + (size_t)slot * (WBM * WBN) + wave * 64 + lane;
#pragma unroll
            for (int q = 0; q < 4; q++)
#pragma unroll
                for (int b = 0; b < NB; b++)
#pragma unroll
                    for (int g = 0; g < 4; g++) {
                        const f32x4 v = src[((q * NB + b) * 4 + g) * 256];
                        yacc[q][b][4 * g + 0] = v.x; yacc[q][b][4 * g + 1] = v.y;
                        yacc[q][b][4 * g + 2] = v.z; yacc[q][b][4 * g + 3] = v.w;
                    }
            // the compiler's own wait for these loads belongs HERE, in front of the drain below, not in front of their first
            // use at the end of the first plane, where it would drain the ring once per plane
#pragma unroll
            for (int q = 0; q < 4; q++)
#pragma unroll
                for (int b = 0; b < NB; b++) asm volatile("" : "+v"(yacc[q][b]));
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    int cur = 0;
    [[maybe_unused]] int left = (xe - xb) * nk;     // RING 3: steps from the current one to the end of the item
    for (int xi = xb; xi < xe; xi++) {
#pragma unroll
        for (int b = 0; b < NB; b++)
#pragma unroll
            for (int r = 0; r < 16; r++) tmp[b][r] = 0.f;
        if constexpr (RING == 3) {
            for (int kc = 0; kc < nk; kc++, left--) {
                // this step's operands have landed (the loads of the step after it may still be out), and every wave is past
                // its reads of the step before: its stage takes step s + 2
                if (left > 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(AG + BG) : "memory");
                else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __syncthreads();
                const unsigned a_cur = a_lane + cur * (WBM * 32 * 4);
                const unsigned b_cur = b_lane + cur * (WBN * 32 * 4);
                frag_read(0, a_cur + chb[0], b_cur + chb[0]);
                if (left > 2) dma_step(cur == 0 ? 2 : cur - 1);     // (cur + 2) % 3, under the latency of the first fragment read
                frag_wait(0);
#pragma unroll
                for (int kk = 0; kk < 4; kk++) {
                    const int sl = kk & 1;
                    if (kk + 1 < 4) frag_read(sl ^ 1, a_cur + chb[kk + 1], b_cur + chb[kk + 1]);
#pragma unroll
                    for (int e = 0; e < 4; e++)
#pragma unroll
                        for (int b = 0; b < NB; b++)
                            tmp[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[sl][e], bv[sl][b][e], tmp[b], 0, 0, 0);
                    if (kk + 1 < 4) frag_wait(sl ^ 1);
                }
                cur = cur == 2 ? 0 : cur + 1;
            }
        } else
        for (int kc = 0; kc < nk; kc++) {
            const unsigned a_cur = a_lane + cur * (WBM * 32 * 4);
            const unsigned b_cur = b_lane + cur * (WBN * 32 * 4);
            frag_read(0, a_cur + chb[0], b_cur + chb[0]);
            if (xi < xe - 1 || kc + 1 < nk) dma_step(cur ^ 1);  // issued under the latency of the first fragment read
            frag_wait(0);
#pragma unroll
            for (int kk = 0; kk < 4; kk++) {
                const int sl = kk & 1;
                if (kk + 1 < 4) frag_read(sl ^ 1, a_cur + chb[kk + 1], b_cur + chb[kk + 1]);
#pragma unroll
                for (int e = 0; e < 4; e++)
#pragma unroll
                    for (int b = 0; b < NB; b++)
                        tmp[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[sl][e], bv[sl][b][e], tmp[b], 0, 0, 0);
                if (kk + 1 < 4) frag_wait(sl ^ 1);
            }
            // the next step's operands have landed, and every wave is past its reads of this one
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            cur ^= 1;
        }
        // y[a][b] += AT[a][i] AT[b][j] M[i][j]: the coefficients are -1, 0 or 1 (wave-uniform), so the fused multiply-add is
        // an exact signed add and the loop over xi stays a loop
        const int i = xi >> 2, j = xi & 3;
#pragma unroll
        for (int a = 0; a < 2; a++)
#pragma unroll
            for (int bq = 0; bq < 2; bq++) {
                const float c = (float)(wino_at(a, i) * wino_at(bq, j));
#pragma unroll
                for (int b = 0; b < NB; b++)
#pragma unroll
                    for (int r = 0; r < 16; r++) yacc[a * 2 + bq][b][r] = __builtin_fmaf(c, tmp[b][r], yacc[a * 2 + bq][b][r]);
            }
    }

    // RING 3: the last step took its barrier BEFORE its reads; the read-out slabs (and the next item's first stages) lie in
    // stages that another wave may still be reading
    if constexpr (RING == 3) __syncthreads();
    if constexpr (PERS) {
        if (xe < 16) {
            // head of a tile: the four accumulator sets in their register layout (16-byte stores), then the flag
            f32x4* dst = reinterpret_cast<f32x4*>(p.sk_ws) + (size_t)slot * (WBM * WBN) + wave * 64 + lane;
#pragma unroll
            for (int q = 0; q < 4; q++)
#pragma unroll
                for (int b = 0; b < NB; b++)
#pragma unroll
                    for (int g = 0; g < 4; g++) {
                        f32x4 v;
                        v.x = yacc[q][b][4 * g + 0]; v.y = yacc[q][b][4 * g + 1];
                        v.z = yacc[q][b][4 * g + 2]; v.w = yacc[q][b][4 * g + 3];
                        dst[((q * NB + b) * 4 + g) * 256] = v;
                    }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            if (tid == 0) {
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __hip_atomic_store(p.sk_flags + slot, p.sk_epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            return;
        }
    }

    // ---- read-out.  Accumulator layout: column = lane & 31 = channel, rows (r & 3) + 8 (r >> 2) + 4 (lane >> 5) = tiles; a
    // wave transposes one 32 x 32 block at a time through a private 4 KiB slab (the staging buffers are idle: every wave
    // passed the loop's last barrier) so that the stores are 16-byte pieces of NHWC rows
    float* slab = smem + wave * 1024;
    const int vrow = lane >> 3, vcol = (lane & 7) * 4;
    long long prow[4];      // element offset of the tile's top-left output pixel in y, -1: tile beyond the launch
    int pw[4], pflag[4];    // map width; bit 0: column 2 tw + 1 inside the map, bit 1: row 2 th + 1 inside
#pragma unroll
    for (int it = 0; it < 4; it++) {
        const int tl = m0 + wm * 32 + it * 8 + vrow;
        prow[it] = -1; pw[it] = 0; pflag[it] = 0;
        if (tl < p.nt) {
            const WinoTile t = wino_tile(p.sg, p.tile0 + tl);
            const int H = p.sg.H[t.seg], W = p.sg.W[t.seg];
            prow[it] = ((long long)p.sg.r0[t.seg] + ((long long)t.n * H + t.h) * W + t.w) * p.Cout;
            pw[it] = W;
            pflag[it] = (t.w + 1 < W ? 1 : 0) | (t.h + 1 < H ? 2 : 0);
        }
    }
    float* __restrict__ yout = p.y;
#pragma unroll
    for (int b = 0; b < NB; b++) {
        const int co = n0 + wn * 32 * NB + b * 32 + li;
        const bool cok = co < p.Cout;
        const float sc = (p.scale && cok) ? p.scale[co] : 1.f;
        const float sh = (p.shift && cok) ? p.shift[co] : 0.f;
        const int cv = n0 + wn * 32 * NB + b * 32 + vcol;
#pragma unroll
        for (int q = 0; q < 4; q++) {
#pragma unroll
            for (int r = 0; r < 16; r++) {
                float o = yacc[q][b][r];
                if (p.scale) o = o * sc;
                slab[((r & 3) + 8 * (r >> 2) + 4 * lh) * 32 + li] = o + sh;
            }
            __builtin_amdgcn_s_waitcnt(0xc07f);
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int it = 0; it < 4; it++) {
                float4 o = *reinterpret_cast<const float4*>(slab + (it * 8 + vrow) * 32 + vcol);
                if (p.relu) { o.x = fmaxf(o.x, 0.f); o.y = fmaxf(o.y, 0.f); o.z = fmaxf(o.z, 0.f); o.w = fmaxf(o.w, 0.f); }
                const bool in_map = ((q & 1) == 0 || (pflag[it] & 1)) && ((q & 2) == 0 || (pflag[it] & 2));
                if (prow[it] >= 0 && in_map && cv < p.Cout)
                    *reinterpret_cast<float4*>(yout + prow[it] + (long long)((q >> 1) * pw[it] + (q & 1)) * p.Cout + cv) = o;
            }
            __builtin_amdgcn_s_waitcnt(0xc07f);
            __builtin_amdgcn_wave_barrier();
        }
    }
#endif
}

// PERS = false: one workgroup per workgroup tile.  PERS = true: the persistent launch of at most the resident workgroups;
// workgroup b owns one contiguous range of the launch's (workgroup tile x xi plane) iteration space, cut into the items
// sk_items[first .. first + count), (first, count) = sk_items[b] (sk_table_ranges, conv_igemm_bf16.hip: the ranges follow
// xcd_remap like the plain launch's tiles, so the column tiles of a row block stay on one XCD): the head of the tile the
// range ends in (published at once: nobody waits long for it), its whole tiles, and last the tail of the tile it starts in.
template <int WBM, int WBN, int WNW, bool PERS = false, int RING = 2>
__global__ __launch_bounds__(256, 2) void wino_gemm_kernel(WinoGemmParams p) {
#if defined(__HIP_DEVICE_COMPILE__)
    static_assert(WBM % 32 == 0 && (WBM / 32) * WNW == 4 && (WBN == 32 * WNW || WBN == 64 * WNW), "four waves of 32 x 32 NB");
    static_assert(RING == 2 || RING == 3, "two or three LDS stages");
    static_assert(RING * (WBM * 32 + WBN * 32) >= 4 * 1024, "the read-out slabs live in the staging buffers");
    __shared__ __attribute__((aligned(16))) float smem[RING * (WBM * 32 + WBN * 32)];     // 64 x 128: 48 KiB with two stages of A and B
    if constexpr (PERS) {
        const int4 range = p.sk_items[blockIdx.x];      // wave-uniform: scalar loads
        const int first = __builtin_amdgcn_readfirstlane(range.x), count = __builtin_amdgcn_readfirstlane(range.y);
        for (int i = 0; i < count; i++) {
            // the read-out slabs and the last step of the item before live in the staging buffers: every wave is past
            // them before the next item's first DMA lands
            if (i > 0) __syncthreads();
            const int4 item = p.sk_items[first + i];
            wino_gemm_item<WBM, WBN, WNW, true, RING>(p, smem, __builtin_amdgcn_readfirstlane(item.x),
                                                __builtin_amdgcn_readfirstlane(item.y), __builtin_amdgcn_readfirstlane(item.z),
                                                __builtin_amdgcn_readfirstlane(item.w));
        }
    } else {
        // the Cout / WBN column tiles of one row block side by side on one XCD: V is fetched from HBM once
        wino_gemm_item<WBM, WBN, WNW, false, RING>(p, smem, xcd_remap(blockIdx.x, p.tiles_m * p.tiles_n), 0, 16, 0);
    }
#endif
}

// host side: the tile table of a segment list; 0 or BRCNN_EINVAL
int wino_segs(WinoSegs& sg, int batch, int num_segments, const int* heights_host, const int* widths_host) {
    if (batch <= 0 || num_segments <= 0 || num_segments > BRCNN_MAX_LEVELS || !heights_host || !widths_host) return BRCNN_EINVAL;
    sg = {};
    sg.nseg = num_segments;
    sg.batch = batch;
    long long tiles = 0, rows = 0;
    for (int s = 0; s < num_segments; s++) {
        const int H = heights_host[s], W = widths_host[s];
        if (H <= 0 || W <= 0 || H >= 4096 || W >= 4096) return BRCNN_EINVAL;
        sg.H[s] = H; sg.W[s] = W; sg.TH[s] = (H + 1) / 2; sg.TW[s] = (W + 1) / 2;
        sg.t0[s] = (int)tiles; sg.r0[s] = (int)rows;
        tiles += (long long)batch * sg.TH[s] * sg.TW[s];
        rows += (long long)batch * H * W;
        if (rows > 0x7fffffffLL / 4) return BRCNN_EINVAL;
    }
    for (int s = num_segments; s <= BRCNN_MAX_LEVELS; s++) { sg.t0[s] = (int)tiles; sg.r0[s] = (int)rows; }
    return 0;
}

}  // namespace

// host-side tile count of a segment list (the workspace holds 16 planes of tiles x cin floats); 0 on a bad argument
BRCNN_API size_t brcnn_conv3x3_winograd_f32_multi_workspace_bytes(int batch, int num_segments, const int* heights_host,
                                                                  const int* widths_host, int cin) {
    WinoSegs sg;
    if (cin <= 0 || wino_segs(sg, batch, num_segments, heights_host, widths_host)) return 0;
    return (size_t)16 * (size_t)sg.t0[num_segments] * (size_t)cin * sizeof(float);
}

BRCNN_API int brcnn_winograd_filter_f32(const void* w, void* u, int cout, int cin, int kh, int kw, int dtype, void* stream) {
    if (!w || !u || dtype != BRCNN_DT_F32 || kh != 3 || kw != 3 || cin <= 0 || cout <= 0 || (cin % 32) || (cout % 64) ||
        (long long)cout * cin * 64 >= 0x7fffffffLL)
        return BRCNN_EINVAL;
    hipLaunchKernelGGL(wino_filter_kernel, dim3((cout * cin + 255) / 256), dim3(256), 0, (hipStream_t)stream, (const float*)w,
                       (float*)u, cout, cin);
    BRCNN_LAUNCH_CHECK();
    return 0;
}

namespace {

// The persistent form of one GEMM launch, or wgs = 0: the plain launch.  The grid is at most the resident workgroups of the
// persistent kernel (occupancy query x CUs, queried once per tile), fewer per CU where the launch has fewer workgroup tiles
// than that (floor(tiles / CUs), one at least: every range then still holds a whole tile's worth of planes), under the
// hooks' caps; policy (-16, 1) asks the measured rule, (-16, 2) takes whatever the schedule allows.  Stream capture, fewer
// workgroup tiles than workgroups and a hand-over area beyond the stream's workspace all give the plain launch
// (sk_plan_ranges).  0, or the error of an earlier launch's lost hand-over
int g_wino_cus = 0;
template <int WBM, int WBN, int WNW, int RING>
int wino_occupancy(int& occ) {
    static int cached = -1;
    if (cached < 0) {
        int n = 0;
        BRCNN_HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, (const void*)wino_gemm_kernel<WBM, WBN, WNW, true, RING>, 256, 0));
        if (g_wino_cus == 0) {
            int dev = 0;
            hipDeviceProp_t prop;
            BRCNN_HIP_CHECK(hipGetDevice(&dev));
            BRCNN_HIP_CHECK(hipGetDeviceProperties(&prop, dev));
            g_wino_cus = prop.multiProcessorCount;
        }
        cached = n;
    }
    occ = cached;
    return 0;
}

template <int RING>
int wino_occupancy_of(int variant, int& occ) {
    return variant == 2 ? wino_occupancy<32, 128, 4, RING>(occ) : variant == 3 ? wino_occupancy<64, 64, 2, RING>(occ)
                                                                               : wino_occupancy<64, 128, 2, RING>(occ);
}

int wino_plan(WinoGemmParams& p, int variant, int ring, hipStream_t s, int& wgs) {
    wgs = 0;
    const int mode = brcnn::g_policy.f32_winograd_sk;
    if (mode == 0) return 0;
    int occ = 0;
    if (const int rc = ring == 3 ? wino_occupancy_of<3>(variant, occ) : wino_occupancy_of<2>(variant, occ)) return rc;
    const int cus = g_wino_cus;
    const long long tiles = (long long)p.tiles_m * p.tiles_n;
    int per_cu = occ;
    if (brcnn::g_policy.f32_winograd_sk_per_cu > 0 && brcnn::g_policy.f32_winograd_sk_per_cu < per_cu) per_cu = brcnn::g_policy.f32_winograd_sk_per_cu;
    if (per_cu <= 0 || cus <= 0) return 0;
    if (tiles < (long long)per_cu * cus) per_cu = tiles / cus > 1 ? (int)(tiles / cus) : 1;
    if (mode == 1 && !brcnn::wino_persistent_rule(tiles > 0x7fffffffLL ? 0x7fffffff : (int)tiles, 16, cus, per_cu)) return 0;
    long long slots = (long long)per_cu * cus;
    if (brcnn::g_policy.f32_winograd_sk_wgs > 0 && brcnn::g_policy.f32_winograd_sk_wgs < slots) slots = brcnn::g_policy.f32_winograd_sk_wgs;
    const int wbm = variant == 2 ? 32 : 64, wbn = variant == 3 ? 64 : 128;
    SkRangePlan k;
    if (const int rc = sk_plan_ranges(k, tiles, 16, (int)slots, (size_t)4 * wbm * wbn * sizeof(float), s)) return rc;
    if (k.wgs <= 0) return 0;
    p.sk_items = k.items; p.sk_ws = k.ws; p.sk_flags = k.flags; p.sk_epoch = k.epoch; p.sk_err = k.err;
    p.sk_spin_limit = k.spin_limit;
    wgs = k.wgs;
    return 0;
}

template <bool PERS, int RING>
void wino_launch(int variant, const dim3& grid, hipStream_t s, const WinoGemmParams& p) {
    if (variant == 2) hipLaunchKernelGGL((wino_gemm_kernel<32, 128, 4, PERS, RING>), grid, dim3(256), 0, s, p);
    else if (variant == 3) hipLaunchKernelGGL((wino_gemm_kernel<64, 64, 2, PERS, RING>), grid, dim3(256), 0, s, p);
    else hipLaunchKernelGGL((wino_gemm_kernel<64, 128, 2, PERS, RING>), grid, dim3(256), 0, s, p);
}

// transform + GEMM launch pairs of one call; `variant` 1 / 2 / 3 as listed at wino_gemm_kernel.  0 or BRCNN_EINVAL; the caller
// has checked the layer form and counts the launch
int wino_run(const void* x, const void* u, const void* gn_stats, const float* gamma, const float* beta, int groups, int relu_in,
             const float* scale, const float* shift, int relu, void* y, void* workspace, size_t workspace_bytes, WinoGemmParams& p,
             int num_segments, int cin, int cout, int variant, void* stream) {
    const int tiles = p.sg.t0[num_segments];
    if ((long long)p.sg.r0[num_segments] * (cin > cout ? cin : cout) * 4 >= 0x7fffffffLL) return BRCNN_EINVAL;
    if (workspace_bytes < (size_t)16 * tiles * cin * sizeof(float)) return BRCNN_EINVAL;
    const int wbm = variant == 2 ? 32 : 64, wbn = variant == 3 ? 64 : 128;
    // chunks of whole workgroup row blocks; more of them where the V planes of one would pass the 2 GiB of a buffer descriptor
    int chunks = brcnn::g_policy.f32_winograd_chunks;
    while ((long long)16 * ((tiles + chunks - 1) / chunks + WBM_MAX) * cin * 4 >= 0x7fffffffLL) chunks *= 2;
    const int per = ((tiles + chunks - 1) / chunks + WBM_MAX - 1) / WBM_MAX * WBM_MAX;
    hipStream_t s = (hipStream_t)stream;
    p.v = (const float*)workspace; p.u = (const float*)u; p.scale = scale; p.shift = shift; p.y = (float*)y;
    p.u_bytes = (unsigned)((long long)cout * cin * 64);
    p.Cin = cin; p.Cout = cout; p.relu = relu;
    p.tiles_n = (cout + wbn - 1) / wbn;
    for (int t0 = 0; t0 < tiles; t0 += per) {
        const int nt = tiles - t0 < per ? tiles - t0 : per;
        const long long th = (long long)nt * (cin >> 2);
        hipLaunchKernelGGL(wino_input_kernel, dim3((unsigned)((th + 255) / 256)), dim3(256), 0, s, (const float*)x, (float*)workspace,
                           p.sg, t0, nt, cin, (const double*)gn_stats, gamma, beta, groups, relu_in);
        BRCNN_LAUNCH_CHECK();
        p.tile0 = t0; p.nt = nt;
        p.v_bytes = (unsigned)((long long)16 * nt * cin * 4);
        p.tiles_m = (nt + wbm - 1) / wbm;
        // the LDS ring: the measured rule or the hook (-16, 42 / 43)
        const int ring = brcnn::g_policy.f32_winograd_ring ? brcnn::g_policy.f32_winograd_ring
                                                           : brcnn::wino_ring_rule(p.tiles_m * p.tiles_n, cin);
        brcnn::g_counters.f32_winograd_last_ring = ring;
        // each launch pair plans for itself: its own epoch of the stream's flags, its own range table
        int wgs = 0;
        if (const int rc = wino_plan(p, variant, ring, s, wgs)) return rc;
        if (wgs > 0) {
            if (ring == 3) wino_launch<true, 3>(variant, dim3(wgs), s, p);
            else wino_launch<true, 2>(variant, dim3(wgs), s, p);
            BRCNN_LAUNCH_CHECK();
            brcnn::count(brcnn::g_counters.f32_winograd_sk_launches);
            brcnn::g_counters.f32_winograd_sk_last_wgs = wgs;
            continue;
        }
        const dim3 grid(p.tiles_m * p.tiles_n);
        if (ring == 3) wino_launch<false, 3>(variant, grid, s, p);
        else wino_launch<false, 2>(variant, grid, s, p);
        BRCNN_LAUNCH_CHECK();
    }
    return 0;
}

}  // namespace

BRCNN_API int brcnn_conv3x3_winograd_f32_multi(const void* x, const void* u, const void* gn_stats, const float* gamma,
                                               const float* beta, int groups, int relu_in, const float* scale,
                                               const float* shift, int relu, void* y, void* workspace, size_t workspace_bytes,
                                               int batch, int num_segments, const int* heights_host, const int* widths_host,
                                               int cin, int cout, int kh, int kw, int stride, int pad, int dtype, void* stream) {
    if (!x || !u || !y || !workspace || dtype != BRCNN_DT_F32 || kh != 3 || kw != 3 || stride != 1 || pad != 1 || cin <= 0 ||
        cout <= 0 || (cin % 32) || (cout % 64) || (long long)cout * cin * 64 >= 0x7fffffffLL)
        return BRCNN_EINVAL;
    if (gn_stats && (!gamma || !beta || groups <= 0 || cin % groups)) return BRCNN_EINVAL;
    WinoGemmParams p = {};
    if (wino_segs(p.sg, batch, num_segments, heights_host, widths_host)) return BRCNN_EINVAL;
    // the tower's tile: the measured rule (64 x 128) or the hook (-16, 20 + v)
    const int variant = brcnn::g_policy.f32_winograd_tower_gemm ? brcnn::g_policy.f32_winograd_tower_gemm
                                                                : brcnn::wino_tower_gemm_rule(p.sg.t0[num_segments], cout);
    const int st = wino_run(x, u, gn_stats, gamma, beta, groups, relu_in, scale, shift, relu, y, workspace, workspace_bytes, p,
                            num_segments, cin, cout, variant, stream);
    if (st) return st;
    brcnn::count(brcnn::g_counters.f32_winograd_launches);
    brcnn::g_counters.f32_winograd_tiles = p.sg.t0[num_segments];
    brcnn::g_counters.f32_winograd_tower_variant = variant;
    return 0;
}

// One frozen conv + folded-BN / bias (+ ReLU) layer, (batch, height, width, cin) -> (batch, height, width, cout), in the same
// form: the single-layer route of blocks.conv_bn_act_nhwc.  The GEMM tile comes from brcnn::wino_gemm_variant (policy.hip:
// the measured rule or the forcing hook (-14, 20 + v)).  Like the entry above it accepts every shape of the layer form and
// never falls back: brcnn_winograd_layer_route says beforehand whether the policy sends a layer here.  Counted apart from the
// tower's launches ((-14, 10): launches, (-14, 11): GEMM variant of the last one).
BRCNN_API int brcnn_conv3x3_winograd_f32_layer(const void* x, const void* u, const float* scale, const float* shift, int relu,
                                               void* y, void* workspace, size_t workspace_bytes, int batch, int height, int width,
                                               int cin, int cout, int kh, int kw, int stride, int pad, int dtype, void* stream) {
    if (!x || !u || !y || !workspace || dtype != BRCNN_DT_F32 || kh != 3 || kw != 3 || stride != 1 || pad != 1 || cin <= 0 ||
        cout <= 0 || (cin % 32) || (cout % 64) || (long long)cout * cin * 64 >= 0x7fffffffLL)
        return BRCNN_EINVAL;
    WinoGemmParams p = {};
    if (wino_segs(p.sg, batch, 1, &height, &width)) return BRCNN_EINVAL;
    const int variant = brcnn::wino_gemm_variant(p.sg.t0[1], cout);
    const int st = wino_run(x, u, nullptr, nullptr, nullptr, 0, 0, scale, shift, relu, y, workspace, workspace_bytes, p, 1, cin,
                            cout, variant, stream);
    if (st) return st;
    brcnn::count(brcnn::g_counters.f32_winograd_layer_launches);
    brcnn::g_counters.f32_winograd_layer_variant = variant;
    return 0;
}
