// Device-side pieces the input-gradient kernels share (inputgrad.hip: field_input_grad_kernel per sample, train_render_ray_grad_kernel per ray):
// the trilinear derivative of one hash level applied to its part of dX, and the Jacobian of the degree-4 SH.
#pragma once
#include "field_dev.h"

MNF_DT_BEGIN

constexpr int kMaxHeadWidth = 64;     // W / 2 at W = 128
#ifndef MNF_GRAD_LEVELS
#define MNF_GRAD_LEVELS 4
#endif
// hash levels per group of gathers: 4 (the forward's group) = 234 VGPRs, two waves per SIMD; 2 = 126 VGPRs, four waves per SIMD, measured 4 % slower
// (profiles/input_grad_levels_ab.txt)
constexpr int kGradLevels = MNF_GRAD_LEVELS;
static_assert(16 % kGradLevels == 0, "whole groups");

// d(feature)/d(frac) of one level applied to the level's feature gradient g: with D[c] = dot(g, entry of corner c) (c = bx + 2 by + 4 bz)
//   x: sum_{by,bz} wy wz (D[1,by,bz] - D[0,by,bz]), likewise y and z; times d(frac)/d(xn) = scale.  fp32 throughout, whatever the forward's blend
// precision was (straight-through, as the oracle's).
__device__ __forceinline__ void level_grad(const LevelMeta m, const float xn[3], const LevelPrep &p, const tab4 (&v)[8], const float4 g, float (&acc)[3]) {
    float D[8];
#pragma unroll
    for (int c = 0; c < 8; ++c)
        D[c] = __builtin_fmaf((float)v[c][3], g.w, __builtin_fmaf((float)v[c][2], g.z, __builtin_fmaf((float)v[c][1], g.y, (float)v[c][0] * g.x)));
    // the fractions exactly as hash_prep formed them
    const float px = __builtin_fmaf(m.scale, xn[0], 0.5f), py = __builtin_fmaf(m.scale, xn[1], 0.5f);
    const float fx = px - floorf(px), fy = py - floorf(py);
    const float wx[2] = {1.0f - fx, fx}, wy[2] = {1.0f - fy, fy};
    float gx = 0.f, gy = 0.f, gz = 0.f;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            gx = __builtin_fmaf(wy[a] * p.wz[b], D[1 + 2 * a + 4 * b] - D[2 * a + 4 * b], gx);      // a = by, b = bz
            gy = __builtin_fmaf(wx[a] * p.wz[b], D[a + 2 + 4 * b] - D[a + 4 * b], gy);              // a = bx, b = bz
            const float wxy = a ? p.wxy[b].y : p.wxy[b].x;                                          // a = bx, b = by
            gz = __builtin_fmaf(wxy, D[a + 2 * b + 4] - D[a + 2 * b], gz);
        }
    acc[0] = __builtin_fmaf(m.scale, gx, acc[0]);
    acc[1] = __builtin_fmaf(m.scale, gy, acc[1]);
    acc[2] = __builtin_fmaf(m.scale, gz, acc[2]);
}

// (gx, gy, gz) = J^T s: the Jacobian of the 16 polynomials of sh4 (field_dev.h) at direction d, column by column, applied to dL/dSH = s.
// The forward's argument: 2u - 1 with u = (d + 1) / 2, chain factor 1.
__device__ __forceinline__ void sh4_jacobian_t(const float *d, const float (&s)[16], float &gx, float &gy, float &gz) {
    const float x = ((d[0] + 1.0f) / 2.0f) * 2.0f - 1.0f;
    const float y = ((d[1] + 1.0f) / 2.0f) * 2.0f - 1.0f;
    const float z = ((d[2] + 1.0f) / 2.0f) * 2.0f - 1.0f;
    const float x2 = x * x, y2 = y * y, z2 = z * z;
    constexpr float c1 = 0.48860251190291987f, c2 = 1.0925484305920792f, c3 = 0.94617469575755997f, c5 = 0.54627421529603959f,
                    c6 = 0.59004358992664352f, c7 = 2.8906114426405538f, c8 = 0.45704579946446572f, c9 = 0.3731763325901154f,
                    c10 = 1.4453057213202769f;
    gx = -c1 * s[3] + c2 * y * s[4] - c2 * z * s[7] + 2.0f * c5 * x * s[8] - 6.0f * c6 * x * y * s[9] + c7 * y * z * s[10]
         + c8 * (1.0f - 5.0f * z2) * s[13] + 2.0f * c10 * x * z * s[14] + 3.0f * c6 * (y2 - x2) * s[15];
    gy = -c1 * s[1] + c2 * x * s[4] - c2 * z * s[5] - 2.0f * c5 * y * s[8] + 3.0f * c6 * (y2 - x2) * s[9] + c7 * x * z * s[10]
         + c8 * (1.0f - 5.0f * z2) * s[11] - 2.0f * c10 * y * z * s[14] + 6.0f * c6 * x * y * s[15];
    gz = c1 * s[2] - c2 * y * s[5] + 2.0f * c3 * z * s[6] - c2 * x * s[7] + c7 * x * y * s[10] - 10.0f * c8 * y * z * s[11]
         + c9 * (15.0f * z2 - 3.0f) * s[12] - 10.0f * c8 * x * z * s[13] + c10 * (x2 - y2) * s[14];
}

MNF_DT_END
