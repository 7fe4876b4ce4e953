// The tail the *_decode_levels kernels of the dense heads share (dense_head.hip, fcos_head.hip, atss_head.hip): what
// happens to candidate slot t of image b, class c, once its box is decoded.
#pragma once
#include "common.h"

// clip to the image (max_shape (B, 2) [h, w]), `/ scale_factor` ((B, 4) or NULL), the box / score / label / valid stores and
// the count of valid candidates per image.  `ok`: the candidate passes score_thr.  Every lane of the calling loop
// iteration must get here (the ballots).
__device__ __forceinline__ void store_candidate(long long t, int b, int c, float ox1, float oy1, float ox2, float oy2,
                                                float score, bool ok, const float* __restrict__ max_shape,
                                                const float* __restrict__ scale_factor, float* __restrict__ boxes,
                                                float* __restrict__ scores, int64_t* __restrict__ labels,
                                                uint8_t* __restrict__ valid, int* __restrict__ n_valid) {
    const float mh = max_shape[2 * b], mw = max_shape[2 * b + 1];
    ox1 = ox1 < 0.f ? 0.f : ox1; ox1 = ox1 > mw ? mw : ox1;
    oy1 = oy1 < 0.f ? 0.f : oy1; oy1 = oy1 > mh ? mh : oy1;
    ox2 = ox2 < 0.f ? 0.f : ox2; ox2 = ox2 > mw ? mw : ox2;
    oy2 = oy2 < 0.f ? 0.f : oy2; oy2 = oy2 > mh ? mh : oy2;
    if (scale_factor) {
        const float* sf = scale_factor + 4 * b;
        ox1 = ox1 / sf[0]; oy1 = oy1 / sf[1]; ox2 = ox2 / sf[2]; oy2 = oy2 / sf[3];
    }
    *reinterpret_cast<float4*>(boxes + (size_t)t * 4) = make_float4(ox1, oy1, ox2, oy2);
    scores[t] = score;
    labels[t] = c;
    valid[t] = ok ? 1 : 0;
    // an integer count (the order of the additions does not matter), one atomic per wave and image instead of one
    // per candidate: the lanes that share the first active lane's image are counted with a ballot
    const unsigned long long active = __ballot(1);
    const int first = __ffsll((long long)active) - 1;
    const int b_first = __shfl(b, first, WAVE);
    const unsigned long long same = __ballot(ok && b == b_first);
    if ((int)(threadIdx.x & (WAVE - 1)) == first && same) atomicAdd(n_valid + b_first, __popcll(same));
    if (ok && b != b_first) atomicAdd(n_valid + b, 1);
}
