// The library's one random generator on the device: Philox4x32-10 (Salmon et al., SC'11), held to known answers by the occupancy refresh's
// pinned draws (tests/test_gpu_occupancy.py) and the pose draw's (tests/test_gpu_localize.py).
//
// Contract: philox4x32_10(ctr, k0, k1) is the ten-round bijection of the 128-bit counter under the 64-bit key (k0 low, k1 high); the four words
// of the result are independent uniform 32-bit draws.  Every user keys it with the caller's 64-bit seed and spends the counter on what the
// draw belongs to, with a word that names the stream, so no two streams of the library share a counter:
//   occupancy.hip   (element low, element high, kind 0 | 1 | 2, step)
//   trainstep.hip   (ray, 0, 7, 0)                      the stratified jitter of a ray's near plane
//   localize.hip    (ray, view, iteration, "pose")      a view's pixel draw
// unit_float(w) is the 24-bit float (w & 0xFFFFFF) * 2^-24 in [0, 1): every value is exact in fp32.  An integer below n is drawn as
// floor(w * n / 2^32) in 64-bit arithmetic by the callers.
#pragma once
#include <cstdint>

#include <hip/hip_runtime.h>

namespace mnf {

struct U4 { uint32_t x, y, z, w; };

__device__ __forceinline__ U4 philox4x32_10(U4 ctr, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * ctr.x, p1 = (uint64_t)0xCD9E8D57u * ctr.z;
        ctr = {(uint32_t)(p1 >> 32) ^ ctr.y ^ k0, (uint32_t)p1, (uint32_t)(p0 >> 32) ^ ctr.w ^ k1, (uint32_t)p0};
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return ctr;
}

__device__ __forceinline__ float unit_float(uint32_t w) { return (float)(w & 0xFFFFFFu) * 5.9604644775390625e-08f; }

}  // namespace mnf
