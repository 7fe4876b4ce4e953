// Training-mode BatchNorm (resnet.py with norm_eval=False: F.batch_norm(training=True)) over (rows, C) NHWC tensors in
// fp32 / bf16 / fp16; statistics and parameters fp32.
//   forward   mean[c] = sum_r z / rows,  var[c] = sum_r (z - mean)^2 / rows  (biased),  rstd = 1 / sqrt(var + eps)
//             scale = gamma rstd,  shift = beta - mean scale   -> the apply pass is brcnn_bn_act_forward (bn_act.hip)
//             running_mean <- (1 - m) running_mean + m mean,   running_var <- (1 - m) running_var + m var rows / (rows - 1)
//   backward  dpre = dout * (out > 0),  xh = (z - mean) rstd
//             dbeta = sum_r dpre,  dgamma = sum_r dpre xh
//             dz = gamma rstd (dpre - dbeta / rows - xh dgamma / rows),  dres = dpre
// HBM-bound streams, 16 bytes per lane.  Reduction scheme, the same for the forward statistics and for dgamma / dbeta:
//   * grid (row strips, channel chunks); block 256 threads = RL row lanes x CW channel vectors.  A lane walks the rows
//     r0 + rl, r0 + rl + RL, ... of its strip and sums in fp32 over chains of at most FOLD = 16 rows; every chain is folded
//     into a double.  Everything after is double: the RL row lanes through LDS in lane order, one (sum a, sum b) pair per
//     strip and channel to the workspace, and a second launch that adds the strips in a fixed order (64 strip lanes,
//     then the 64 lane sums in order).  No atomics: the same bits on every run.
//   * the forward sums are SHIFTED: with the pivot p[c] = z[0][c] (row 0 of the tensor, the same for every strip, so the
//     partials simply add) the lanes accumulate sum (z - p) and sum (z - p)^2, and the second stage forms
//         mean = p + S1 / rows,   var = S2 / rows - (S1 / rows)^2        in double.
//     The cancellation in var is that of (mean - p)^2 against var, not of mean^2 against var: with delta = mean - p,
//         |d var| <= 51 u (delta^2 + var),   |d mean| <= 16 u sqrt(delta^2 + var) + u |mean|,   u = 2^-24
//     (tests/bn_ref64.py derives the constants).  p is one sample of the channel, so delta^2 is of the order of var
//     whatever mean^2 / var is; a constant channel has z - p == 0 and var == 0 exactly.
//   * the backward sums dpre (z - mean), never sum dpre z - mean sum dpre.
#include <type_traits>
#include "common.h"

namespace {

template <typename T> struct Vec;
template <> struct Vec<float> { static constexpr int N = 4; };
template <> struct Vec<bf16_t> { static constexpr int N = 8; };
template <> struct Vec<f16_t> { static constexpr int N = 8; };

__device__ __forceinline__ void ldv(const float* p, float v[4]) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
}
__device__ __forceinline__ void ldv(const bf16_t* p, float v[8]) {
    const uint4 u = *reinterpret_cast<const uint4*>(p);
    const unsigned w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
    for (int e = 0; e < 4; e++) {
        v[2 * e] = __uint_as_float(w[e] << 16);
        v[2 * e + 1] = __uint_as_float(w[e] & 0xffff0000u);
    }
}
__device__ __forceinline__ void ldv(const f16_t* p, float v[8]) {
    const uint4 u = *reinterpret_cast<const uint4*>(p);
    const unsigned w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
    for (int e = 0; e < 4; e++) {
        v[2 * e] = brcnn_h2f((unsigned short)(w[e] & 0xffffu));
        v[2 * e + 1] = brcnn_h2f((unsigned short)(w[e] >> 16));
    }
}
__device__ __forceinline__ void stv(float* p, const float v[4]) {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
}
__device__ __forceinline__ void stv(bf16_t* p, const float v[8]) {
    uint4 u;
    u.x = brcnn_pk2b(v[0], v[1]);
    u.y = brcnn_pk2b(v[2], v[3]);
    u.z = brcnn_pk2b(v[4], v[5]);
    u.w = brcnn_pk2b(v[6], v[7]);
    *reinterpret_cast<uint4*>(p) = u;
}
__device__ __forceinline__ void stv(f16_t* p, const float v[8]) {
    uint4 u;
    u.x = brcnn_pk2h(v[0], v[1]);
    u.y = brcnn_pk2h(v[2], v[3]);
    u.z = brcnn_pk2h(v[4], v[5]);
    u.w = brcnn_pk2h(v[6], v[7]);
    *reinterpret_cast<uint4*>(p) = u;
}
__device__ __forceinline__ float ld1(const float* p) { return *p; }
__device__ __forceinline__ float ld1(const bf16_t* p) { return brcnn_b2f(*p); }
__device__ __forceinline__ float ld1(const f16_t* p) { return brcnn_h2f(p->v); }

constexpr int FOLD = 16;        // rows per fp32 chain (tests/bn_ref64.py: FOLD)
constexpr int U = 4;            // rows in flight per lane: the loads of a group are issued before its first use

// the RL row lanes of a workgroup, combined in lane order; `a` then `b` through one LDS array
template <int V>
__device__ __forceinline__ void strip_partials(double (*red)[V], const double a[V], const double b[V],
                                               double* __restrict__ partial, int C, int CW, int cv, int cvn) {
    const int cl = threadIdx.x % CW, rl = threadIdx.x / CW, RL = 256 / CW;
#pragma unroll
    for (int which = 0; which < 2; which++) {
#pragma unroll
        for (int e = 0; e < V; e++) red[threadIdx.x][e] = which ? b[e] : a[e];
        __syncthreads();
        if (rl == 0 && cv < cvn) {
#pragma unroll
            for (int e = 0; e < V; e++) {
                double t = 0.0;
                for (int k = 0; k < RL; k++) t += red[k * CW + cl][e];
                partial[((size_t)blockIdx.x * 2 + which) * C + cv * V + e] = t;      // [strip][a | b][C]
            }
        }
        __syncthreads();
    }
}

// forward statistics, first stage: per strip and channel sum (z - p), sum (z - p)^2 with p = z[0][c]
template <typename T>
__global__ __launch_bounds__(256) void bn_train_stats_kernel(const T* __restrict__ z, double* __restrict__ partial,
                                                            long long rows, int C, int rows_per_block, int CW) {
    constexpr int V = Vec<T>::N;
    __shared__ double red[256][V];
    const int cvn = C / V;
    const int cv = blockIdx.y * CW + (threadIdx.x % CW);
    const int rl = threadIdx.x / CW, RL = 256 / CW;
    const long long r0 = (long long)blockIdx.x * rows_per_block;
    const long long r1 = min(rows, r0 + rows_per_block);
    double d1[V], d2[V];
#pragma unroll
    for (int e = 0; e < V; e++) { d1[e] = 0.0; d2[e] = 0.0; }
    if (cv < cvn) {
        float p[V], s1[V], s2[V];
        ldv(z + (long long)cv * V, p);
        auto acc = [&](auto n_c, long long r) {
            constexpr int N = decltype(n_c)::value;
            float x[N][V];
#pragma unroll
            for (int u = 0; u < N; u++) ldv(z + ((r + (long long)u * RL) * cvn + cv) * V, x[u]);
#pragma unroll
            for (int u = 0; u < N; u++)
#pragma unroll
                for (int e = 0; e < V; e++) {
                    const float d = x[u][e] - p[e];
                    s1[e] += d;
                    s2[e] += d * d;
                }
        };
        long long r = r0 + rl;
        while (r < r1) {
#pragma unroll
            for (int e = 0; e < V; e++) { s1[e] = 0.f; s2[e] = 0.f; }
            int g = 0;
            for (; g < FOLD / U && r + (long long)(U - 1) * RL < r1; g++, r += (long long)RL * U)
                acc(std::integral_constant<int, U>{}, r);
            if (g < FOLD / U)           // fewer than U rows are left: the strip's last chain ends with them
                for (; r < r1; r += RL) acc(std::integral_constant<int, 1>{}, r);
#pragma unroll
            for (int e = 0; e < V; e++) { d1[e] += (double)s1[e]; d2[e] += (double)s2[e]; }
        }
    }
    strip_partials<V>(red, d1, d2, partial, C, CW, cv, cvn);
}

// second stage of the statistics + finalize: 16 columns x 64 strip lanes per workgroup
template <typename T>
__global__ __launch_bounds__(1024) void bn_train_finalize_kernel(
    const double* __restrict__ partial, const T* __restrict__ z, const float* __restrict__ gamma,
    const float* __restrict__ beta, float eps, float momentum, float* __restrict__ running_mean,
    float* __restrict__ running_var, float* __restrict__ save_mean, float* __restrict__ save_rstd,
    float* __restrict__ batch_var, float* __restrict__ scale, float* __restrict__ shift, int strips, long long rows, int C) {
    __shared__ double red[2][64][16];
    const int col = blockIdx.x * 16 + (threadIdx.x & 15), sl = threadIdx.x >> 4;
    double a = 0.0, b = 0.0;
    if (col < C)
        for (int s = sl; s < strips; s += 64) {
            a += partial[((size_t)s * 2 + 0) * C + col];
            b += partial[((size_t)s * 2 + 1) * C + col];
        }
    red[0][sl][threadIdx.x & 15] = a;
    red[1][sl][threadIdx.x & 15] = b;
    __syncthreads();
    if (sl == 0 && col < C) {
        double ta = 0.0, tb = 0.0;
#pragma unroll
        for (int k = 0; k < 64; k++) { ta += red[0][k][threadIdx.x]; tb += red[1][k][threadIdx.x]; }
        const double n = (double)rows;
        const double m1 = ta / n;
        const double mean = (double)ld1(z + col) + m1;
        double var = tb / n - m1 * m1;
        if (var < 0.0) var = 0.0;
        const float mean_f = (float)mean;
        const float rstd_f = (float)(1.0 / sqrt(var + (double)eps));
        const float sc = gamma[col] * rstd_f;
        save_mean[col] = mean_f;
        save_rstd[col] = rstd_f;
        if (batch_var) batch_var[col] = (float)var;
        scale[col] = sc;
        shift[col] = beta[col] - mean_f * sc;
        const double m = (double)momentum;
        running_mean[col] = (float)((1.0 - m) * (double)running_mean[col] + m * mean);
        running_var[col] = (float)((1.0 - m) * (double)running_var[col] + m * (var * (n / (n - 1.0))));
    }
}

// backward, reduce pass: per strip and channel sum dpre, sum dpre (z - mean)
template <typename T>
__global__ __launch_bounds__(256) void bn_train_bwd_reduce_kernel(const T* __restrict__ dout, const T* __restrict__ out,
                                                                 const T* __restrict__ z,
                                                                 const float* __restrict__ save_mean,
                                                                 double* __restrict__ partial, long long rows, int C,
                                                                 int rows_per_block, int CW) {
    constexpr int V = Vec<T>::N;
    __shared__ double red[256][V];
    const int cvn = C / V;
    const int cv = blockIdx.y * CW + (threadIdx.x % CW);
    const int rl = threadIdx.x / CW, RL = 256 / CW;
    const long long r0 = (long long)blockIdx.x * rows_per_block;
    const long long r1 = min(rows, r0 + rows_per_block);
    double d1[V], d2[V];
#pragma unroll
    for (int e = 0; e < V; e++) { d1[e] = 0.0; d2[e] = 0.0; }
    if (cv < cvn) {
        float mn[V], s1[V], s2[V];
#pragma unroll
        for (int e = 0; e < V; e++) mn[e] = save_mean[cv * V + e];
        // (the mask source is a launch constant, as in bn_act_bwd_kernel)
        auto acc = [&](auto n_c, auto out_c, long long r) {
            constexpr int N = decltype(n_c)::value;
            constexpr bool OUT = decltype(out_c)::value;
            float g[N][V], o[OUT ? N : 1][V], x[N][V];
#pragma unroll
            for (int u = 0; u < N; u++) {
                const long long idx = ((r + (long long)u * RL) * cvn + cv) * V;
                ldv(dout + idx, g[u]);
                if constexpr (OUT) ldv(out + idx, o[u]);
                ldv(z + idx, x[u]);
            }
#pragma unroll
            for (int u = 0; u < N; u++)
#pragma unroll
                for (int e = 0; e < V; e++) {
                    float d = g[u][e];
                    if constexpr (OUT) d = o[u][e] > 0.f ? d : 0.f;
                    s1[e] += d;
                    s2[e] += d * (x[u][e] - mn[e]);
                }
        };
        auto strip = [&](auto out_c) {
            long long r = r0 + rl;
            while (r < r1) {
#pragma unroll
                for (int e = 0; e < V; e++) { s1[e] = 0.f; s2[e] = 0.f; }
                int g = 0;
                for (; g < FOLD / U && r + (long long)(U - 1) * RL < r1; g++, r += (long long)RL * U)
                    acc(std::integral_constant<int, U>{}, out_c, r);
                if (g < FOLD / U)
                    for (; r < r1; r += RL) acc(std::integral_constant<int, 1>{}, out_c, r);
#pragma unroll
                for (int e = 0; e < V; e++) { d1[e] += (double)s1[e]; d2[e] += (double)s2[e]; }
            }
        };
        if (out) strip(std::true_type{});
        else strip(std::false_type{});
    }
    strip_partials<V>(red, d1, d2, partial, C, CW, cv, cvn);
}

// second stage of the backward sums: dbeta = sum dpre, dgamma = rstd sum dpre (z - mean)
__global__ __launch_bounds__(1024) void bn_train_bwd_finalize_kernel(const double* __restrict__ partial,
                                                                    const float* __restrict__ save_rstd,
                                                                    float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                                    int strips, int C) {
    __shared__ double red[2][64][16];
    const int col = blockIdx.x * 16 + (threadIdx.x & 15), sl = threadIdx.x >> 4;
    double a = 0.0, b = 0.0;
    if (col < C)
        for (int s = sl; s < strips; s += 64) {
            a += partial[((size_t)s * 2 + 0) * C + col];
            b += partial[((size_t)s * 2 + 1) * C + col];
        }
    red[0][sl][threadIdx.x & 15] = a;
    red[1][sl][threadIdx.x & 15] = b;
    __syncthreads();
    if (sl == 0 && col < C) {
        double ta = 0.0, tb = 0.0;
#pragma unroll
        for (int k = 0; k < 64; k++) { ta += red[0][k][threadIdx.x]; tb += red[1][k][threadIdx.x]; }
        dbeta[col] = (float)ta;
        dgamma[col] = (float)(tb * (double)save_rstd[col]);
    }
}

// backward, write pass.  The launch makes gridDim.x * 256 a multiple of C / V (bn_act_fwd_kernel's rule): a thread meets
// the same channels in every iteration and holds their coefficients in registers
template <typename T>
__global__ __launch_bounds__(256) void bn_train_bwd_write_kernel(const T* __restrict__ dout, const T* __restrict__ out,
                                                                const T* __restrict__ z, const float* __restrict__ gamma,
                                                                const float* __restrict__ save_mean,
                                                                const float* __restrict__ save_rstd,
                                                                const float* __restrict__ dgamma,
                                                                const float* __restrict__ dbeta, T* __restrict__ dz,
                                                                T* __restrict__ dres, long long rows, int C, float inv_rows) {
    constexpr int V = Vec<T>::N;
    const int cvn = C / V;
    const long long total = rows * cvn;
    const long long first = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int c0 = (int)(first % cvn) * V;
    float mn[V], rs[V], gs[V], k1[V], k2[V];
#pragma unroll
    for (int e = 0; e < V; e++) {
        mn[e] = save_mean[c0 + e];
        rs[e] = save_rstd[c0 + e];
        gs[e] = gamma[c0 + e] * rs[e];
        k1[e] = dbeta[c0 + e] * inv_rows;
        k2[e] = dgamma[c0 + e] * inv_rows;
    }
    for (long long idx = first; idx < total; idx += (long long)gridDim.x * blockDim.x) {
        float g[V], o[V], x[V];
        ldv(dout + idx * V, g);
        if (out) ldv(out + idx * V, o);
        ldv(z + idx * V, x);
#pragma unroll
        for (int e = 0; e < V; e++) {
            const float d = (!out || o[e] > 0.f) ? g[e] : 0.f;
            g[e] = d;
            const float xh = (x[e] - mn[e]) * rs[e];
            x[e] = gs[e] * (d - k1[e] - xh * k2[e]);
        }
        stv(dz + idx * V, x);
        if (dres) stv(dres + idx * V, g);
    }
}

struct Plan { int V, CW, chunks; long long strips, rpb; };

// bn_act.hip's strip rule: short maps (rows < 16384) split the channels too (64 vectors per workgroup, ~1024 workgroups of
// >= 32 rows); long maps keep up to 256 vectors per workgroup and ~512 strips of >= 64 rows
bool plan(int64_t rows, int channels, int dtype, Plan* pl) {
    if (rows < 2 || channels <= 0 || !brcnn_elem_ok(dtype)) return false;
    const int V = dtype == BRCNN_DT_F32 ? 4 : 8;
    if (channels % V) return false;
    const int cvn = channels / V;
    if (cvn & (cvn - 1)) return false;                // channel-vector count a power of two
    // rows * C elements and their byte offsets (doubles in the workspace included) within int64
    if ((uint64_t)rows > (uint64_t)INT64_MAX / ((uint64_t)channels * 16)) return false;
    const bool short_map = rows < 16384;
    const int cw_max = short_map ? 64 : 256;
    const int wg_target = short_map ? 1024 : 512;
    const int min_rows = short_map ? 32 : 64;
    int CW = 1;
    while (CW < cvn && CW < cw_max) CW <<= 1;
    pl->V = V;
    pl->CW = CW;
    pl->chunks = cvn / CW;
    long long strips = wg_target / pl->chunks;
    if (strips < 1) strips = 1;
    long long rpb = (rows + strips - 1) / strips;
    if (rpb < min_rows) rpb = min_rows;
    pl->rpb = rpb;
    pl->strips = (rows + rpb - 1) / rpb;
    return true;
}

int write_grid(long long total, int cvn) {
    long long g = (total + 255) / 256;
    if (g > 2048) g = 2048;
    if (g < 1) g = 1;
    long long step = 1;
    while ((step * 256) % cvn) step++;
    return (int)((g + step - 1) / step * step);
}

}  // namespace

BRCNN_API size_t brcnn_bn_train_workspace_bytes(int64_t rows, int channels, int dtype) {
    Plan pl;
    if (!plan(rows, channels, dtype, &pl)) return 0;
    return (size_t)pl.strips * 2 * channels * sizeof(double);
}

BRCNN_API int brcnn_bn_train_stats(const void* z, const float* gamma, const float* beta, float eps, float momentum,
                                   float* running_mean, float* running_var, float* save_mean, float* save_rstd,
                                   float* batch_var, float* scale, float* shift, void* workspace, size_t workspace_bytes,
                                   int64_t rows, int channels, int dtype, void* stream) {
    Plan pl;
    if (!z || !gamma || !beta || !running_mean || !running_var || !save_mean || !save_rstd || !scale || !shift ||
        !workspace || !(eps >= 0.f) || !plan(rows, channels, dtype, &pl))
        return BRCNN_EINVAL;
    if (workspace_bytes < (size_t)pl.strips * 2 * channels * sizeof(double) || ((uintptr_t)workspace & 7)) return BRCNN_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)pl.strips, pl.chunks), fgrid((channels + 15) / 16);
    double* part = (double*)workspace;
#define BRCNN_BN_TRAIN_STATS(T)                                                                                          \
    do {                                                                                                                 \
        hipLaunchKernelGGL(bn_train_stats_kernel<T>, grid, dim3(256), 0, s, (const T*)z, part, (long long)rows, channels, \
                           (int)pl.rpb, pl.CW);                                                                          \
        BRCNN_LAUNCH_CHECK();                                                                                            \
        hipLaunchKernelGGL(bn_train_finalize_kernel<T>, fgrid, dim3(1024), 0, s, (const double*)part, (const T*)z, gamma, \
                           beta, eps, momentum, running_mean, running_var, save_mean, save_rstd, batch_var, scale, shift, \
                           (int)pl.strips, (long long)rows, channels);                                                   \
    } while (0)
    if (dtype == BRCNN_DT_F32) BRCNN_BN_TRAIN_STATS(float);
    else if (dtype == BRCNN_DT_BF16) BRCNN_BN_TRAIN_STATS(bf16_t);
    else BRCNN_BN_TRAIN_STATS(f16_t);
#undef BRCNN_BN_TRAIN_STATS
    BRCNN_LAUNCH_CHECK();
    return 0;
}

BRCNN_API int brcnn_bn_train_backward(const void* dout, const void* out, const void* z, const float* gamma,
                                      const float* save_mean, const float* save_rstd, void* dz, void* dres, float* dgamma,
                                      float* dbeta, void* workspace, size_t workspace_bytes, int64_t rows, int channels,
                                      int relu, int dtype, void* stream) {
    Plan pl;
    if (!dout || !z || !gamma || !save_mean || !save_rstd || !dz || !dgamma || !dbeta || !workspace ||
        (relu && !out) || !plan(rows, channels, dtype, &pl))
        return BRCNN_EINVAL;
    if (workspace_bytes < (size_t)pl.strips * 2 * channels * sizeof(double) || ((uintptr_t)workspace & 7)) return BRCNN_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const void* mask = relu ? out : nullptr;
    const dim3 grid((unsigned)pl.strips, pl.chunks), fgrid((channels + 15) / 16);
    const int cvn = channels / pl.V;
    const int wgrid = write_grid((long long)rows * cvn, cvn);
    const float inv_rows = (float)(1.0 / (double)rows);
    double* part = (double*)workspace;
#define BRCNN_BN_TRAIN_BWD(T)                                                                                            \
    do {                                                                                                                 \
        hipLaunchKernelGGL(bn_train_bwd_reduce_kernel<T>, grid, dim3(256), 0, s, (const T*)dout, (const T*)mask,          \
                           (const T*)z, save_mean, part, (long long)rows, channels, (int)pl.rpb, pl.CW);                 \
        BRCNN_LAUNCH_CHECK();                                                                                            \
        hipLaunchKernelGGL(bn_train_bwd_finalize_kernel, fgrid, dim3(1024), 0, s, (const double*)part, save_rstd, dgamma, \
                           dbeta, (int)pl.strips, channels);                                                             \
        BRCNN_LAUNCH_CHECK();                                                                                            \
        hipLaunchKernelGGL(bn_train_bwd_write_kernel<T>, dim3(wgrid), dim3(256), 0, s, (const T*)dout, (const T*)mask,    \
                           (const T*)z, gamma, save_mean, save_rstd, (const float*)dgamma, (const float*)dbeta, (T*)dz,   \
                           (T*)dres, (long long)rows, channels, inv_rows);                                               \
    } while (0)
    if (dtype == BRCNN_DT_F32) BRCNN_BN_TRAIN_BWD(float);
    else if (dtype == BRCNN_DT_BF16) BRCNN_BN_TRAIN_BWD(bf16_t);
    else BRCNN_BN_TRAIN_BWD(f16_t);
#undef BRCNN_BN_TRAIN_BWD
    BRCNN_LAUNCH_CHECK();
    return 0;
}
