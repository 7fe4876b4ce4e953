// COCO bbox / proposal evaluation on the device (evaluation.DeviceCOCOeval): the three stages of COCOeval
// (evaluation.py: evaluateImg, the per-category score order, accumulate) as a fixed number of launches.
//
//   match       one wave per (category, image) pair; lane a*T + t runs the serial greedy matching of area range a at IoU
//               threshold t over the pair's detections (descending score, cut to maxDets[-1]) and ground truths, the IoU of
//               (d, g) recomputed on the fly in fp64.  Its "ground truth taken" bits are lane-private words in LDS.
//   order       LSD radix sort (8-bit digits) of all detections by (category, descending score); stable, so ties keep the
//               pair-major input order = the host's (image, in-pair rank) order.  Ranks inside a digit come from wave
//               ballots and per-tile counters: no atomic decides a position.
//   accumulate  one workgroup per (threshold, category, area range, maxDet): a forward count, then a backward sweep that
//               rebuilds the cumulative tp / fp counts, the precision, its running maximum from the right, and drops the
//               values at the recall look-up points.
//
// Every floating-point operation is an fp64 add / multiply / divide or a comparison in the host's order (the build has
// -ffp-contract=off), every sum is an integer count: the results are the host evaluator's bit for bit.
#include "common.h"

#define CE_THREADS 256
#define CE_WAVES (CE_THREADS / WAVE)
#define CE_MAX_GT 1024                  // ground truths of one pair (taken bits: CE_MAX_GT / 32 words per lane)
#define CE_MAX_REC 1024                 // recall look-up points
#define CE_TILE 1024                    // sort: elements per wave and pass
#define CE_EPS 2.220446049250313e-16    // np.spacing(1)

typedef unsigned long long u64;

// ------------------------------------------------------------------------------------------------ match
__device__ __forceinline__ double ce_iou(double dx, double dy, double dw, double dh, double da, const double *g, bool crowd) {
    const double gx = g[0], gy = g[1], gw = g[2], gh = g[3];
    const double w = fmin(dx + dw, gx + gw) - fmax(dx, gx);
    const double h = fmin(dy + dh, gy + gh) - fmax(dy, gy);
    const double inter = (w > 0 && h > 0) ? w * h : 0.0;
    const double uni = crowd ? da : da + gw * gh - inter;
    return inter > 0 ? inter / uni : 0.0;
}

__global__ __launch_bounds__(CE_THREADS) void ce_match_kernel(
    const double *__restrict__ gt_box, const double *__restrict__ gt_area, const uint8_t *__restrict__ gt_flags,
    const int *__restrict__ gt_off, const float *__restrict__ det, const int *__restrict__ det_off, int n_pairs, int n_img,
    const double *__restrict__ iou_thrs, int T, const double *__restrict__ area_rng, int A, uint16_t *__restrict__ dtm,
    uint16_t *__restrict__ dtig, uint8_t *__restrict__ gtig, int *__restrict__ npig, int *__restrict__ det_rank,
    u64 *__restrict__ det_key) {
    __shared__ unsigned taken[CE_WAVES][(CE_MAX_GT / 32) * WAVE];
    const int wave = threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
    const int pair = blockIdx.x * CE_WAVES + wave;
    if (pair >= n_pairs) return;
    const int g0 = gt_off[pair], G = gt_off[pair + 1] - g0;
    const int d0 = det_off[pair], D = det_off[pair + 1] - d0;
    if ((G == 0 && D == 0) || G < 0 || D < 0 || G > CE_MAX_GT) return;      // (the entry point refuses such a table)
    const int k = pair / n_img;
    const bool active = lane < A * T;
    const int a = active ? lane / T : 0, t = active ? lane % T : 0;
    const double lo = area_rng[2 * a], hi = area_rng[2 * a + 1];
    const double thr = fmin(iou_thrs[t], 1 - 1e-10);
    unsigned *mine = &taken[wave][lane];                // word w of this lane: mine[w * WAVE]

    // per ground truth: the ignore bit of every area range; per area range: the number of ground truths that count
    for (int g = lane; g < G; g += WAVE) {
        const double ar = gt_area[g0 + g];
        const bool crowd = gt_flags[g0 + g] & 1;
        unsigned m = 0;
        for (int x = 0; x < A; x++) m |= (unsigned)(crowd || ar < area_rng[2 * x] || ar > area_rng[2 * x + 1]) << x;
        gtig[g0 + g] = (uint8_t)m;
    }
    if (active && t == 0) {
        int cnt = 0;
        for (int g = 0; g < G; g++) cnt += !((gt_flags[g0 + g] & 1) || gt_area[g0 + g] < lo || gt_area[g0 + g] > hi);
        if (cnt) atomicAdd(&npig[k * A + a], cnt);      // (an integer count: the order of arrival cannot change it)
    }
    // per detection: in-pair rank and the sort key (category, descending score; -0 sorts as +0)
    for (int d = lane; d < D; d += WAVE) {
        const float s = det[(size_t)(d0 + d) * 5 + 4] + 0.0f;
        unsigned b = __float_as_uint(s);
        b = ~(b ^ ((b & 0x80000000u) ? 0xFFFFFFFFu : 0x80000000u));
        det_rank[d0 + d] = d;
        det_key[d0 + d] = ((u64)(unsigned)k << 32) | b;
    }
    const int words = (G + 31) / 32;
    for (int w = 0; w < words; w++) mine[w * WAVE] = 0;

    for (int d = 0; d < D; d++) {
        const float *p = det + (size_t)(d0 + d) * 5;
        const double dx = (double)p[0], dy = (double)p[1];
        const double dw = (double)p[2] - dx, dh = (double)p[3] - dy;
        const double da = dw * dh;
        bool matched = false, ignored = false;
        if (active) {
            double iou = thr;
            int m = -1;
            bool m_ig = false;
            for (int pass = 0; pass < 2; pass++) {      // ground truths that count first, then the ignored ones
                if (pass == 1 && m >= 0) break;         // a match that counts is held and the ignored ones begin
                for (int g = 0; g < G; g++) {
                    const uint8_t fl = gt_flags[g0 + g];
                    const bool crowd = fl & 1;
                    const double ar = gt_area[g0 + g];
                    const bool ig = crowd || ar < lo || ar > hi;
                    if ((int)ig != pass) continue;
                    if (!crowd && ((mine[(g >> 5) * WAVE] >> (g & 31)) & 1)) continue;
                    const double v = ce_iou(dx, dy, dw, dh, da, gt_box + (size_t)(g0 + g) * 4, crowd);
                    if (v < iou) continue;
                    iou = v;
                    m = g;
                    m_ig = ig;
                }
            }
            if (m >= 0) {
                mine[(m >> 5) * WAVE] |= 1u << (m & 31);
                matched = (gt_flags[g0 + m] >> 1) & 1;  // the host stores the ground truth's id and tests its truth value
                ignored = m_ig;
            }
            ignored = ignored || (!matched && (da < lo || da > hi));
        }
        const u64 bm = __ballot(matched), bi = __ballot(ignored);
        if (active && t == 0) {
            const unsigned mask = (1u << T) - 1;
            dtm[(size_t)(d0 + d) * A + a] = (uint16_t)((bm >> (a * T)) & mask);
            dtig[(size_t)(d0 + d) * A + a] = (uint16_t)((bi >> (a * T)) & mask);
        }
    }
}

// ------------------------------------------------------------------------------------------------ order
__global__ __launch_bounds__(CE_THREADS) void ce_sort_hist_kernel(const u64 *__restrict__ key, int n, int shift, int n_tiles,
                                                                 unsigned *__restrict__ counts) {
    __shared__ unsigned h[CE_WAVES][256];
    const int wave = threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
    const int tile = blockIdx.x * CE_WAVES + wave;
    for (int i = lane; i < 256; i += WAVE) h[wave][i] = 0;
    __syncthreads();
    if (tile < n_tiles) {
        const int base = tile * CE_TILE;
        for (int r = 0; r < CE_TILE / WAVE; r++) {
            const int i = base + r * WAVE + lane;
            if (i < n) atomicAdd(&h[wave][(unsigned)(key[i] >> shift) & 255u], 1u);    // (integer counts)
        }
    }
    __syncthreads();
    if (tile < n_tiles)
        for (int i = lane; i < 256; i += WAVE) counts[(size_t)i * n_tiles + tile] = h[wave][i];
}

// exclusive scan of `m` counters in place, one workgroup
__global__ __launch_bounds__(1024) void ce_sort_scan_kernel(unsigned *__restrict__ counts, int m) {
    __shared__ unsigned part[1024];
    const int tid = threadIdx.x;
    const int per = (m + 1023) / 1024;
    const int b = tid * per, e = min(b + per, m);
    unsigned s = 0;
    for (int i = b; i < e; i++) s += counts[i];
    part[tid] = s;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        const unsigned v = tid >= off ? part[tid - off] : 0;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    unsigned run = part[tid] - s;
    for (int i = b; i < e; i++) {
        const unsigned c = counts[i];
        counts[i] = run;
        run += c;
    }
}

__global__ __launch_bounds__(CE_THREADS) void ce_sort_scatter_kernel(const u64 *__restrict__ key_in, const unsigned *__restrict__ val_in,
                                                                    int n, int shift, int n_tiles, const unsigned *__restrict__ offs,
                                                                    u64 *__restrict__ key_out, unsigned *__restrict__ val_out) {
    __shared__ unsigned base[CE_WAVES][256];
    const int wave = threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
    const int tile = blockIdx.x * CE_WAVES + wave;
    const bool live = tile < n_tiles;
    if (live)
        for (int i = lane; i < 256; i += WAVE) base[wave][i] = offs[(size_t)i * n_tiles + tile];
    __syncthreads();
    const u64 below = lane ? (~0ull >> (WAVE - lane)) : 0ull;
    for (int r = 0; r < CE_TILE / WAVE; r++) {
        const int i = tile * CE_TILE + r * WAVE + lane;
        const bool have = live && i < n;
        const u64 kk = have ? key_in[i] : 0;
        const unsigned dg = (unsigned)(kk >> shift) & 255u;
        u64 peers = __ballot(have);
        for (int b = 0; b < 8; b++) {               // the lanes of this round that hold the same digit
            const u64 bb = __ballot((dg >> b) & 1);
            peers &= ((dg >> b) & 1) ? bb : ~bb;
        }
        const unsigned rank = __popcll(peers & below);
        unsigned pos = 0;
        if (have) pos = base[wave][dg] + rank;
        __syncthreads();
        if (have && rank + 1 == (unsigned)__popcll(peers)) base[wave][dg] = pos + 1;   // the last of its digit moves the counter
        __syncthreads();
        if (have) {
            key_out[pos] = kk;
            val_out[pos] = val_in ? val_in[i] : (unsigned)i;
        }
    }
}

// ------------------------------------------------------------------------------------------------ accumulate
struct ce_cnt { int tp, fp, kept; };

__device__ __forceinline__ ce_cnt ce_add(ce_cnt x, ce_cnt y) { return {x.tp + y.tp, x.fp + y.fp, x.kept + y.kept}; }

// inclusive scan over the workgroup from the left; `total` = the sum of all
__device__ __forceinline__ ce_cnt ce_block_scan(ce_cnt v, ce_cnt *wsum, ce_cnt *total) {
    const int wave = threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
    for (int off = 1; off < WAVE; off <<= 1) {
        ce_cnt o = {__shfl_up(v.tp, off), __shfl_up(v.fp, off), __shfl_up(v.kept, off)};
        if (lane >= off) v = ce_add(v, o);
    }
    __syncthreads();
    if (lane == WAVE - 1) wsum[wave] = v;
    __syncthreads();
    ce_cnt pre = {0, 0, 0}, all = {0, 0, 0};
    for (int w = 0; w < CE_WAVES; w++) {
        if (w < wave) pre = ce_add(pre, wsum[w]);
        all = ce_add(all, wsum[w]);
    }
    *total = all;
    return ce_add(v, pre);
}

// inclusive maximum over the workgroup from the RIGHT (thread i gets max of i .. last); returns thread 0's in *first
__device__ __forceinline__ double ce_block_suffix_max(double v, double *wmax, double *first) {
    const int wave = threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
    for (int off = 1; off < WAVE; off <<= 1) {
        const double o = __shfl_down(v, off);
        if (lane + off < WAVE) v = fmax(v, o);
    }
    __syncthreads();
    if (lane == 0) wmax[wave] = v;
    __syncthreads();
    double post = -1.0, all = -1.0;
    for (int w = 0; w < CE_WAVES; w++) {
        if (w > wave) post = fmax(post, wmax[w]);
        all = fmax(all, wmax[w]);
    }
    *first = all;
    return fmax(v, post);
}

__global__ __launch_bounds__(CE_THREADS) void ce_accumulate_kernel(
    const unsigned *__restrict__ order, const int *__restrict__ det_off, int n_img, const float *__restrict__ det,
    const int *__restrict__ det_rank, const uint16_t *__restrict__ dtm, const uint16_t *__restrict__ dtig,
    const int *__restrict__ npig_arr, const double *__restrict__ rec_thrs, const int *__restrict__ max_dets, int T, int R,
    int K, int A, int M, double *__restrict__ precision, double *__restrict__ scores, double *__restrict__ recall) {
    __shared__ int cr[CE_MAX_REC];
    __shared__ double q[CE_MAX_REC], ss[CE_MAX_REC];
    __shared__ ce_cnt wsum[CE_WAVES];
    __shared__ double wmax[CE_WAVES];
    const int tid = threadIdx.x;
    int b = blockIdx.x;
    const int m = b % M; b /= M;
    const int a = b % A; b /= A;
    const int k = b % K; b /= K;
    const int t = b;
    const size_t stride_r = (size_t)K * A * M;
    const size_t o5 = (size_t)t * R * stride_r + ((size_t)k * A + a) * M + m;      // + r * stride_r
    const size_t o4 = (((size_t)t * K + k) * A + a) * M + m;
    const int npig = npig_arr[k * A + a];
    if (npig == 0) {            // nothing to find in this category and range (or no pair at all)
        for (int r = tid; r < R; r += CE_THREADS) {
            precision[o5 + r * stride_r] = -1.0;
            scores[o5 + r * stride_r] = -1.0;
        }
        if (tid == 0) recall[o4] = -1.0;
        return;
    }
    const int s0 = det_off[(size_t)k * n_img], s1 = det_off[(size_t)(k + 1) * n_img];
    const int max_det = max_dets[m];
    const double dn = (double)npig;
    // the smallest true-positive count whose recall reaches each look-up point (npig + 1: none does)
    for (int r = tid; r < R; r += CE_THREADS) {
        const double want = rec_thrs[r];
        int lo = 0, hi = npig + 1;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if ((double)mid / dn >= want) hi = mid; else lo = mid + 1;
        }
        cr[r] = lo;
        q[r] = 0.0;
        ss[r] = 0.0;
    }
    // forward: the totals
    ce_cnt mine = {0, 0, 0};
    for (int j = s0 + tid; j < s1; j += CE_THREADS) {
        const unsigned i = order[j];
        if (det_rank[i] < max_det) {
            const int mt = (dtm[(size_t)i * A + a] >> t) & 1, ig = (dtig[(size_t)i * A + a] >> t) & 1;
            mine.tp += mt & !ig;
            mine.fp += !mt & !ig;
            mine.kept += 1;
        }
    }
    ce_cnt after;
    ce_block_scan(mine, wsum, &after);
    if (tid == 0) recall[o4] = after.kept ? (double)after.tp / dn : 0.0;
    // backward: chunk by chunk from the end, the counts at each element from the totals after the chunk
    double carry = -1.0;
    const int chunks = (s1 - s0 + CE_THREADS - 1) / CE_THREADS;
    for (int c = chunks - 1; c >= 0; c--) {
        const int j = s0 + c * CE_THREADS + tid;
        ce_cnt f = {0, 0, 0};
        double sc = 0.0;
        if (j < s1) {
            const unsigned i = order[j];
            if (det_rank[i] < max_det) {
                const int mt = (dtm[(size_t)i * A + a] >> t) & 1, ig = (dtig[(size_t)i * A + a] >> t) & 1;
                f.tp = mt & !ig;
                f.fp = !mt & !ig;
                f.kept = 1;
                sc = (double)det[(size_t)i * 5 + 4];
            }
        }
        ce_cnt sum;
        ce_cnt inc = ce_block_scan(f, wsum, &sum);
        const int tp = after.tp - sum.tp + inc.tp, fp = after.fp - sum.fp + inc.fp, kept = after.kept - sum.kept + inc.kept;
        const double pr = f.kept ? (double)tp / (((double)fp + (double)tp) + CE_EPS) : -1.0;
        double first;
        const double env = fmax(ce_block_suffix_max(pr, wmax, &first), carry);
        carry = fmax(carry, first);
        after.tp -= sum.tp; after.fp -= sum.fp; after.kept -= sum.kept;
        if (f.kept && (f.tp || kept == 1)) {
            // the look-up points served by this element: those whose count is reached here, and (first kept element)
            // those that ask for recall 0
            for (int pass = 0; pass < 2; pass++) {
                if (pass == 0 ? !f.tp : kept != 1) continue;
                const int want = pass == 0 ? tp : 0;
                int lo = 0, hi = R;
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (cr[mid] >= want) hi = mid; else lo = mid + 1;
                }
                for (int r = lo; r < R && cr[r] == want; r++) {
                    q[r] = env;
                    ss[r] = sc;
                }
            }
        }
    }
    __syncthreads();
    for (int r = tid; r < R; r += CE_THREADS) {
        precision[o5 + r * stride_r] = q[r];
        scores[o5 + r * stride_r] = ss[r];
    }
}

// ------------------------------------------------------------------------------------------------ C ABI
static inline int ce_tiles(int64_t n) { return (int)((n + CE_TILE - 1) / CE_TILE); }
static inline size_t ce_al(size_t b) { return (b + 255) & ~(size_t)255; }

BRCNN_API size_t brcnn_coco_order_workspace_bytes(int64_t num_dets) {
    if (num_dets < 0) return 0;
    const size_t n = (size_t)num_dets;
    return 2 * ce_al(n * sizeof(u64)) + ce_al(n * sizeof(unsigned)) + ce_al((size_t)256 * ce_tiles(num_dets) * sizeof(unsigned)) + 256;
}

BRCNN_API int brcnn_coco_match(const double *gt_box, const double *gt_area, const uint8_t *gt_flags, const int32_t *gt_off,
                               const float *det, const int32_t *det_off, int num_cats, int num_imgs, const double *iou_thrs,
                               int num_thrs, const double *area_rng, int num_areas, int max_gt_per_pair,
                               uint16_t *dt_matched, uint16_t *dt_ignored, uint8_t *gt_ignored, int32_t *num_gt, int32_t *det_rank,
                               uint64_t *det_key, void *stream) {
    if (num_cats < 1 || num_imgs < 1 || num_thrs < 1 || num_thrs > 16 || num_areas < 1 || num_areas > 8 ||
        num_thrs * num_areas > WAVE || max_gt_per_pair < 0 || max_gt_per_pair > CE_MAX_GT || (int64_t)num_cats * num_imgs > 0x7fffffff - CE_WAVES)
        return BRCNN_EINVAL;
    if (!gt_off || !det_off || !iou_thrs || !area_rng || !dt_matched || !dt_ignored || !gt_ignored || !num_gt || !det_rank ||
        !det_key)
        return BRCNN_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    BRCNN_HIP_CHECK(hipMemsetAsync(num_gt, 0, (size_t)num_cats * num_areas * sizeof(int32_t), s));
    const int pairs = num_cats * num_imgs;
    hipLaunchKernelGGL(ce_match_kernel, dim3(brcnn_cdiv(pairs, CE_WAVES)), dim3(CE_THREADS), 0, s, gt_box, gt_area, gt_flags,
                       gt_off, det, det_off, pairs, num_imgs, iou_thrs, num_thrs, area_rng, num_areas, dt_matched, dt_ignored,
                       gt_ignored, num_gt, det_rank, (u64 *)det_key);
    BRCNN_LAUNCH_CHECK();
    return 0;
}

BRCNN_API int brcnn_coco_order(const uint64_t *det_key, int64_t num_dets, int num_cats, uint32_t *order, void *workspace,
                               size_t workspace_bytes, void *stream) {
    if (num_dets < 0 || num_dets > 0x7fffffff - CE_TILE || num_cats < 1 || num_cats > 65536) return BRCNN_EINVAL;
    if (num_dets == 0) return 0;
    if (!det_key || !order || !workspace || workspace_bytes < brcnn_coco_order_workspace_bytes(num_dets)) return BRCNN_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const int n = (int)num_dets, tiles = ce_tiles(num_dets);
    char *w = (char *)(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
    u64 *kb[2];
    kb[0] = (u64 *)w; w += ce_al((size_t)n * sizeof(u64));
    kb[1] = (u64 *)w; w += ce_al((size_t)n * sizeof(u64));
    unsigned *tmp = (unsigned *)w; w += ce_al((size_t)n * sizeof(unsigned));
    unsigned *counts = (unsigned *)w;
    const int passes = num_cats > 256 ? 6 : (num_cats > 1 ? 5 : 4);      // score bytes, then the category's
    const u64 *kin = (const u64 *)det_key;
    const unsigned *vin = nullptr;
    const int blocks = brcnn_cdiv(tiles, CE_WAVES);
    for (int p = 0; p < passes; p++) {
        unsigned *vout = ((passes - 1 - p) % 2 == 0) ? (unsigned *)order : tmp;
        u64 *kout = kb[p % 2];
        hipLaunchKernelGGL(ce_sort_hist_kernel, dim3(blocks), dim3(CE_THREADS), 0, s, kin, n, 8 * p, tiles, counts);
        hipLaunchKernelGGL(ce_sort_scan_kernel, dim3(1), dim3(1024), 0, s, counts, 256 * tiles);
        hipLaunchKernelGGL(ce_sort_scatter_kernel, dim3(blocks), dim3(CE_THREADS), 0, s, kin, vin, n, 8 * p, tiles, counts, kout, vout);
        BRCNN_LAUNCH_CHECK();
        kin = kout;
        vin = vout;
    }
    return 0;
}

BRCNN_API int brcnn_coco_accumulate(const uint32_t *order, const int32_t *det_off, int num_imgs, const float *det,
                                    const int32_t *det_rank, const uint16_t *dt_matched, const uint16_t *dt_ignored,
                                    const int32_t *num_gt, const double *rec_thrs, const int32_t *max_dets, int num_thrs,
                                    int num_recs, int num_cats, int num_areas, int num_max_dets, double *precision,
                                    double *scores, double *recall, void *stream) {
    if (num_thrs < 1 || num_thrs > 16 || num_recs < 1 || num_recs > CE_MAX_REC || num_cats < 1 || num_areas < 1 ||
        num_areas > 8 || num_max_dets < 1 || num_imgs < 1)
        return BRCNN_EINVAL;
    const int64_t blocks = (int64_t)num_thrs * num_cats * num_areas * num_max_dets;
    if (blocks > 0x7fffffff) return BRCNN_EINVAL;
    if (!det_off || !num_gt || !rec_thrs || !max_dets || !precision || !scores || !recall) return BRCNN_EINVAL;
    hipLaunchKernelGGL(ce_accumulate_kernel, dim3((unsigned)blocks), dim3(CE_THREADS), 0, (hipStream_t)stream, order, det_off,
                       num_imgs, det, det_rank, dt_matched, dt_ignored, num_gt, rec_thrs, max_dets, num_thrs, num_recs,
                       num_cats, num_areas, num_max_dets, precision, scores, recall);
    BRCNN_LAUNCH_CHECK();
    return 0;
}
