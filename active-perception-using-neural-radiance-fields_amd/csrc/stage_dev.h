// Staging of a tile's per-pixel logit rows in LDS, shared by the kernels that walk finished renders one pixel per lane
// (eval.hip: eval_views_kernel, frames.hip: frames_views_kernel, infomap.hip: infomap_views_kernel).
#pragma once
#include "common.h"

namespace mnf {

constexpr int kStageBytes = 40960;            // LDS for a tile's logits: leaves room for the kernels' own scratch under 64 KB

// Pixels per tile for C classes at `threads` lanes per workgroup: as many rows of stride C | 1 as kStageBytes holds, at most one per
// lane; 0 when not even one row fits.
inline int stage_tile_pixels(int32_t C, int threads) {
    const int64_t cs = C | 1;
    int64_t tp = kStageBytes / (cs * 4);
    if (tp > threads) tp = threads;
    if (tp >= 4) tp &= ~(int64_t)3;           // tiles of a multiple of four pixels keep every tile of an aligned view 16-byte aligned
    return (int)tp;
}

// Copy the n = np * C contiguous floats at `src` (element e0 of an array whose base is 16-byte aligned iff `vec_ok`) into `stage` as np
// rows of stride Cs = C | 1: 16-byte loads per lane between the first and the last 16-byte boundary, scalar loads before and after (all
// scalar when the base is not aligned).  The odd row stride puts the 32 lanes of an LDS access that reads one column on 32 different banks.
// Every lane of the workgroup calls it; the caller puts a barrier before (the previous tile's rows are read) and after.
template <int kThreads>
__device__ __forceinline__ void stage_rows(float *__restrict__ stage, const float *__restrict__ src, int n, int C, int Cs, int64_t e0, int vec_ok,
                                           int tid) {
    const int head = vec_ok ? min(n, (int)((4 - (e0 & 3)) & 3)) : n;
    const int nvec = (n - head) >> 2;
    if (Cs == C) {
        for (int i = tid; i < head; i += kThreads) stage[i] = src[i];
        for (int q = tid; q < nvec; q += kThreads) {
            const float4 x = *reinterpret_cast<const float4 *>(src + head + 4 * q);
            float *dst = stage + head + 4 * q;
            dst[0] = x.x; dst[1] = x.y; dst[2] = x.z; dst[3] = x.w;
        }
        for (int i = head + 4 * nvec + tid; i < n; i += kThreads) stage[i] = src[i];
    } else {
        for (int i = tid; i < head; i += kThreads) stage[(i / C) * Cs + i % C] = src[i];
        for (int q = tid; q < nvec; q += kThreads) {
            const float4 x = *reinterpret_cast<const float4 *>(src + head + 4 * q);
            const float xs[4] = {x.x, x.y, x.z, x.w};
            int e = head + 4 * q, p = e / C, c = e - p * C;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                stage[p * Cs + c] = xs[k];
                if (++c == C) { c = 0; ++p; }
            }
        }
        for (int i = head + 4 * nvec + tid; i < n; i += kThreads) stage[(i / C) * Cs + i % C] = src[i];
    }
}

// First maximal index of a row of C logits; a NaN counts as the maximum (torch.argmax, np.argmax).  `*best_out` is that logit.
__device__ __forceinline__ int first_argmax(const float *row, int C, float *best_out) {
    float best = row[0];
    int arg = 0;
    for (int c = 1; c < C; ++c) {
        const float x = row[c];
        if (x > best || (x != x && best == best)) { best = x; arg = c; }
    }
    *best_out = best;
    return arg;
}

}  // namespace mnf
