// Sums over a wave and over a workgroup, in a fixed order: the same inputs give the same bits on every run.
//
// wave_sum(x)        the __shfl_down tree over the 64 lanes, offsets 32, 16, .. 1: LANE 0 holds the sum (the other lanes hold partial sums of
//                    no use).  Pairs added: (l, l + 32), then (l, l + 16), ...
// wave_sum_all(x)    the __shfl_xor butterfly, masks 32, 16, .. 1: EVERY lane holds the sum, and all 64 hold the same bits (at every stage the
//                    two lanes of a pair add the same two numbers).
// block_sum<WAVES>(v, s_wave)
//                    a workgroup of WAVES full waves (blockDim.x == 64 * WAVES, one-dimensional): wave_sum_all, the wave leaders' sums through
//                    s_wave[WAVES] in LDS, then the waves added in order 0, 1, .. from 0.0.  Every thread calls it and every thread gets the
//                    sum.  It takes a barrier in front of its stores (s_wave may still be read from a previous call) and one behind them, so
//                    calls can follow one another on the same s_wave.  The loop over the waves stays a loop: it runs once per workgroup, and
//                    unrolled its WAVES loads in flight at once set the register count of a kernel that is small otherwise.
// wave_sum_each(a, b, ..), wave_sum_all_each(a, b, ..)
//                    wave_sum / wave_sum_all of several values at once, in place: one pass over the offsets with every value's shuffle in it,
//                    so the independent chains overlap.
//
// T is whatever the site sums (int, unsigned long long, float, double); the shape of the tree is part of a float sum's value, so a site
// that changes from one form to the other changes its bits.  All lanes of the wave must be active.
#pragma once
#include <hip/hip_runtime.h>

namespace mnf {

template <typename T>
__device__ __forceinline__ T wave_sum(T x) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, 64);
    return x;
}

template <typename T>
__device__ __forceinline__ T wave_sum_all(T x) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) x += __shfl_xor(x, d, 64);
    return x;
}

template <typename... T>
__device__ __forceinline__ void wave_sum_each(T &...x) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) ((x += __shfl_down(x, off, 64)), ...);
}

template <typename... T>
__device__ __forceinline__ void wave_sum_all_each(T &...x) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) ((x += __shfl_xor(x, d, 64)), ...);
}

template <int WAVES>
__device__ __forceinline__ double block_sum(double v, double *s_wave) {
    v = wave_sum_all(v);
    __syncthreads();      // (s_wave may still be read from the previous sum)
    if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = 0.0;
#pragma unroll 1
    for (int w = 0; w < WAVES; ++w) t += s_wave[w];
    return t;
}

}  // namespace mnf
