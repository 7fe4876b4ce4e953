// Batched input front door: Resize -> RandomFlip -> Normalize -> Pad of a whole (augs x images) batch of decoded
// uint8 BGR images in ONE launch (the per-image form and the arithmetic it states: preprocess.hip).
//   read  src block: the B source images back to back, (H_b, W_b, 3) u8 HWC, ragged
//   read  job table: one brcnn_pre_job per (aug, image), device resident
//   write per aug one (B, 3, PH_a, PW_a) fp32 NCHW tensor, EVERY element: pixels, the image's own bottom / right
//         padding and the padding up to the aug's batch shape
// Work split.  A workgroup owns one (job, 64-row band, 128-column band) tile; the flat grid is the sum of the jobs'
// tile counts, and a workgroup finds its job by bisecting the table's `first_block` column (wave-uniform loads).  A
// lane owns 4 consecutive output columns and writes each plane with one 16-byte store, so a half-wave writes 512
// contiguous bytes of a row; the 8 half-waves of the workgroup take rows r, r + 8, ... of the band.  The x sample
// positions and 11-bit coefficients of a lane's 4 columns (double precision, as OpenCV derives them) are computed once
// and reused over its 8 rows; the y coefficients once per row.  Rows and columns of the padding region only store.
// A `pad_w` (or destination offset) that is not a multiple of 4 takes 4-byte stores with a per-column bound instead.
#include "common.h"

namespace {

constexpr int TILE_W = 128, TILE_H = 64, ROW_SLOTS = 8;

struct BatchParams {
    const uint8_t* src;
    float* dst;
    const brcnn_pre_job* jobs;
    int num_jobs, to_rgb;
    float mean[3], stdinv[3];
};

// (identical to preprocess.hip: the two kernels must agree bit for bit)
__device__ __forceinline__ void axis_coeff(int d, double scale, int src, int& s, int& c0, int& c1) {
    float f = (float)(((double)d + 0.5) * scale - 0.5);
    s = (int)floorf(f);
    f -= (float)s;
    if (s < 0) { f = 0.f; s = 0; }
    if (s >= src - 1) { f = 0.f; s = src - 1; }
    c0 = (int)rintf((1.f - f) * 2048.f);
    c1 = (int)rintf(f * 2048.f);
}

typedef float f32x4 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(256) void preprocess_u8_batch_kernel(BatchParams p) {
    const int bid = blockIdx.x;
    int lo = 0, hi = p.num_jobs - 1;
    while (lo < hi) {                                   // last job whose first tile is <= bid
        const int mid = (lo + hi + 1) >> 1;
        if (p.jobs[mid].first_block <= bid) lo = mid; else hi = mid - 1;
    }
    const brcnn_pre_job j = p.jobs[lo];
    const int t = bid - j.first_block;
    const int bands_x = (j.pad_w + TILE_W - 1) / TILE_W;
    const int x0 = (t % bands_x) * TILE_W + (threadIdx.x & 31) * 4;
    const int y0 = (t / bands_x) * TILE_H + (threadIdx.x >> 5);
    if (x0 >= j.pad_w || y0 >= j.pad_h) return;
    const bool vec = ((j.pad_w & 3) == 0) && ((j.dst_off & 3) == 0);
    const size_t plane = (size_t)j.pad_h * j.pad_w;
    float* const out = p.dst + j.dst_off + x0;
    const uint8_t* const img = p.src + j.src_off;
    const size_t row_bytes = (size_t)j.src_w * 3;

    int o0[4], o1[4], a0[4], a1[4];                     // byte offsets of the two taps in a source row, coefficients
    bool live[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int x = x0 + k;
        live[k] = x < j.new_w;
        int sx = 0;
        a0[k] = a1[k] = 0;
        if (live[k]) axis_coeff((j.flip & 1) ? j.new_w - 1 - x : x, j.scale_x, j.src_w, sx, a0[k], a1[k]);
        o0[k] = sx * 3;
        o1[k] = min(sx + 1, j.src_w - 1) * 3;
    }
    const int c_first = p.to_rgb ? 2 : 0, c_step = p.to_rgb ? -1 : 1;

#pragma unroll 1
    for (int y = y0; y < j.pad_h && y < y0 + TILE_H - (int)(threadIdx.x >> 5); y += ROW_SLOTS) {
        float v[3][4];
#pragma unroll
        for (int c = 0; c < 3; c++)
#pragma unroll
            for (int k = 0; k < 4; k++) v[c][k] = 0.f;
        if (y < j.new_h && live[0]) {
            int sy, b0, b1;
            axis_coeff((j.flip & 2) ? j.new_h - 1 - y : y, j.scale_y, j.src_h, sy, b0, b1);
            const uint8_t* r0 = img + (size_t)min(max(sy, 0), j.src_h - 1) * row_bytes;
            const uint8_t* r1 = img + (size_t)min(max(sy + 1, 0), j.src_h - 1) * row_bytes;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                if (!live[k]) continue;
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    const int sc = c_first + c_step * c;
                    const int h0 = (int)r0[o0[k] + sc] * a0[k] + (int)r0[o1[k] + sc] * a1[k];
                    const int h1 = (int)r1[o0[k] + sc] * a0[k] + (int)r1[o1[k] + sc] * a1[k];
                    int q = (((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2;
                    q = min(max(q, 0), 255);
                    v[c][k] = ((float)q - p.mean[c]) * p.stdinv[c];
                }
            }
        }
        float* o = out + (size_t)y * j.pad_w;
        if (vec) {
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const f32x4 q = {v[c][0], v[c][1], v[c][2], v[c][3]};
                *reinterpret_cast<f32x4*>(o + c * plane) = q;
            }
        } else {
#pragma unroll
            for (int k = 0; k < 4; k++) {
                if (x0 + k >= j.pad_w) break;
#pragma unroll
                for (int c = 0; c < 3; c++) o[c * plane + k] = v[c][k];
            }
        }
    }
}

}  // namespace

BRCNN_API int64_t brcnn_preprocess_u8_batch_blocks(int pad_h, int pad_w) {
    if (pad_h <= 0 || pad_w <= 0) return 0;
    return (int64_t)((pad_h + TILE_H - 1) / TILE_H) * ((pad_w + TILE_W - 1) / TILE_W);
}

BRCNN_API int brcnn_preprocess_u8_batch(const uint8_t* src, size_t src_bytes, const brcnn_pre_job* jobs_dev,
                                        const brcnn_pre_job* jobs_host, int num_jobs, float* dst, size_t dst_elems,
                                        const float* mean3_host, const float* std3_host, int to_rgb, void* stream) {
    if (!src || !jobs_dev || !jobs_host || !dst || num_jobs <= 0 || num_jobs > BRCNN_PRE_MAX_JOBS || !mean3_host ||
        !std3_host || ((uintptr_t)dst & 15) || ((uintptr_t)jobs_dev & 7))
        return BRCNN_EINVAL;
    // every row is checked on the host copy before anything is queued: the kernel trusts the table
    int64_t blocks = 0;
    for (int i = 0; i < num_jobs; i++) {
        const brcnn_pre_job& j = jobs_host[i];
        if (j.src_h <= 0 || j.src_w <= 0 || j.new_h <= 0 || j.new_w <= 0 || j.pad_h < j.new_h || j.pad_w < j.new_w ||
            j.flip < 0 || j.flip > 3 || j.src_off < 0 || j.dst_off < 0)
            return BRCNN_EINVAL;
        const uint64_t sbytes = (uint64_t)j.src_h * (uint64_t)j.src_w * 3u;
        const uint64_t delems = (uint64_t)j.pad_h * (uint64_t)j.pad_w * 3u;
        if ((uint64_t)j.src_off > src_bytes || sbytes > src_bytes - (uint64_t)j.src_off) return BRCNN_EINVAL;
        if ((uint64_t)j.dst_off > dst_elems || delems > dst_elems - (uint64_t)j.dst_off) return BRCNN_EINVAL;
        if (j.scale_x != 1.0 / ((double)j.new_w / (double)j.src_w) ||
            j.scale_y != 1.0 / ((double)j.new_h / (double)j.src_h))
            return BRCNN_EINVAL;
        if ((int64_t)j.first_block != blocks) return BRCNN_EINVAL;
        blocks += brcnn_preprocess_u8_batch_blocks(j.pad_h, j.pad_w);
        if (blocks > 0x7fffffff) return BRCNN_EINVAL;
    }
    BatchParams p;
    p.src = src; p.dst = dst; p.jobs = jobs_dev; p.num_jobs = num_jobs; p.to_rgb = to_rgb ? 1 : 0;
    for (int c = 0; c < 3; c++) {
        if (!(std3_host[c] != 0.f)) return BRCNN_EINVAL;
        p.mean[c] = mean3_host[c];
        p.stdinv[c] = (float)(1.0 / (double)std3_host[c]);
    }
    hipLaunchKernelGGL(preprocess_u8_batch_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p);
    BRCNN_LAUNCH_CHECK();
    return 0;
}
