// The skeleton of the passes that walk finished renders of V views of P pixels, one pixel per lane (eval.hip: eval_views_kernel,
// ensemble.hip: ensemble_views_kernel, frames.hip: frames_views_kernel, infomap.hip: infomap_views_kernel).
//
// Work split: a view's pixels are cut into tiles of `tp` pixels, a view's tiles into `nb` contiguous runs, one workgroup of kViewThreads
// lanes per (run, view): grid (nb, V), workgroup b of view v walks tiles [tiles * b / nb, tiles * (b + 1) / nb).  tp depends on C only and nb
// on P and C, so a view's results do not depend on how many views share the call or where it stands.
// Staging: a tile's tp * C logits are one contiguous piece of `sem`; the workgroup copies it to LDS (stage_rows), then lane t works on pixel
// t out of LDS, whose row stride C | 1 is odd, so the 32 lanes of an LDS access that reads one column hit 32 different banks.
// Sums are carried in double: per lane over its pixels, then a shuffle tree per wave, then the four waves in order, then ONE row of K partial
// sums per workgroup in the caller's workspace (store_partials); a finish kernel of one wave per view adds a view's rows in a fixed order
// (sum_partials).  No floating-point atomic anywhere: the same inputs give the same bits.
#pragma once
#include "common.h"
#include "reduce_dev.h"

namespace mnf {

constexpr int kViewThreads = 256;
constexpr int kViewMaxBlocksPerView = 512;
constexpr int kStageBytes = 40960;            // LDS for a tile's logits: leaves room for the kernels' own scratch under 64 KB

struct ViewPlan { int tp; int64_t tiles; int nb; };

// tp >= 1
inline ViewPlan view_plan(int64_t n_pix, int tp) {
    const int64_t tiles = ceil_div(n_pix, tp);
    return {tp, tiles, (int)(tiles < kViewMaxBlocksPerView ? tiles : kViewMaxBlocksPerView)};
}

// Pixels per tile for C classes: as many rows of stride C | 1, at `entry_bytes` of LDS per class entry, as `budget` bytes hold, at most one
// per lane; 0 when not even one row fits.
inline int stage_tile_pixels(int32_t C, int entry_bytes = 4, int budget = kStageBytes) {
    const int64_t cs = C | 1;
    int64_t tp = budget / (cs * entry_bytes);
    if (tp > kViewThreads) tp = kViewThreads;
    if (tp >= 4) tp &= ~(int64_t)3;           // tiles of a multiple of four pixels keep every tile of an aligned view 16-byte aligned
    return (int)tp;
}

// bytes of the caller's workspace: one row of K doubles per workgroup
inline int64_t view_partials_bytes(int32_t n_views, int nb, int K) { return (int64_t)n_views * nb * K * (int64_t)sizeof(double); }

// Copy the n = np * C contiguous floats at `src` (4-byte aligned) into `stage` as np rows of stride Cs = C | 1: 16-byte loads per lane between
// the first and the last 16-byte boundary of the ADDRESS, scalar loads before and after, so a base that is only 4-byte aligned is read wide
// as well and nothing outside [src, src + n) is read.
// Every lane of the workgroup calls it; the caller puts a barrier before (the previous tile's rows are read) and after.
__device__ __forceinline__ void stage_rows(float *__restrict__ stage, const float *__restrict__ src, int n, int C, int Cs, int tid) {
    const int head = min(n, (int)(((16 - (reinterpret_cast<uintptr_t>(src) & 15)) & 15) >> 2));
    const int nvec = (n - head) >> 2;
    if (Cs == C) {
        for (int i = tid; i < head; i += kViewThreads) stage[i] = src[i];
        for (int q = tid; q < nvec; q += kViewThreads) {
            const float4 x = *reinterpret_cast<const float4 *>(src + head + 4 * q);
            float *dst = stage + head + 4 * q;
            dst[0] = x.x; dst[1] = x.y; dst[2] = x.z; dst[3] = x.w;
        }
        for (int i = head + 4 * nvec + tid; i < n; i += kViewThreads) stage[i] = src[i];
    } else {
        for (int i = tid; i < head; i += kViewThreads) stage[(i / C) * Cs + i % C] = src[i];
        for (int q = tid; q < nvec; q += kViewThreads) {
            const float4 x = *reinterpret_cast<const float4 *>(src + head + 4 * q);
            const float xs[4] = {x.x, x.y, x.z, x.w};
            int e = head + 4 * q, p = e / C, c = e - p * C;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                stage[p * Cs + c] = xs[k];
                if (++c == C) { c = 0; ++p; }
            }
        }
        for (int i = head + 4 * nvec + tid; i < n; i += kViewThreads) stage[(i / C) * Cs + i % C] = src[i];
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

// x clamped to [0, 255] and rounded to nearest, ties to even; NaN -> 0, +inf -> 255, -inf -> 0
__device__ __forceinline__ uint8_t sat8(float y) {
    if (!(y > 0.0f)) return 0;                                     // negative, -inf, NaN, zero
    if (y >= 255.0f) return 255;
    return (uint8_t)(int)rintf(y);                                 // round half to even
}

__device__ __forceinline__ uint8_t sat8(double y) {
    if (!(y > 0.0)) return 0;
    if (y >= 255.0) return 255;
    return (uint8_t)(int)rint(y);
}

// The workgroup's row of `partials` from every lane's part[K]: wave_sum (reduce_dev.h) per wave, then the four waves in order.  Every lane of workgroup
// b of view v calls it, once; it holds ONE workgroup barrier, after every lane's last use of `part`'s inputs (eval_views_kernel counts on it).
template <int K>
__device__ __forceinline__ void store_partials(const double (&part)[K], double *__restrict__ partials, int v, int nb, int b, int tid) {
    __shared__ double red[kViewThreads / 64][K];
    const int wave = tid >> 6, lane = tid & 63;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const double w = wave_sum(part[k]);
        if (lane == 0) red[wave][k] = w;
    }
    __syncthreads();
    if (tid < K) {
        double s = red[0][tid];
        for (int w = 1; w < kViewThreads / 64; ++w) s += red[w][tid];
        partials[((int64_t)v * nb + b) * K + tid] = s;
    }
}

// View v's K sums from its nb rows of `partials`, for a finish kernel of one wave per view: lane l adds rows l, l + 64, ... in order, then
// the shuffle tree; lane 0 holds the sums.
template <int K>
__device__ __forceinline__ void sum_partials(const double *__restrict__ partials, int v, int nb, int lane, double (&s)[K]) {
#pragma unroll
    for (int k = 0; k < K; ++k) s[k] = 0.0;
    for (int b = lane; b < nb; b += 64) {
#pragma unroll
        for (int k = 0; k < K; ++k) s[k] += partials[((int64_t)v * nb + b) * K + k];
    }
#pragma unroll
    for (int k = 0; k < K; ++k) s[k] = wave_sum(s[k]);
}

}  // namespace mnf
