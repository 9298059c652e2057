// What the units that work on single pixels share: a pixel's camera ray, a pixel's targets out of the dataset's storage, and a ray's terms of the
// training loss.  Each is promised bit for bit somewhere (tests/golden/raygen.npz, the dataset goldens, tests/test_gpu_localize.py), so each
// exists once, here.
//
// The ray (habitat_to_data.py:274-301), pixel (x, y) of a W x H image, focal length `focal`, row-major 3 x 4 pose m:
//   cam0 = (x - W / 2 + 0.5) / focal,  cam1 = (y - H / 2 + 0.5) / focal * -1,  cam2 = -1
//   d[i] = (cam0 * m[4 i] + cam1 * m[4 i + 1]) + cam2 * m[4 i + 2]            un-normalised; the origin is m[4 i + 3]
// in exactly this order, every operation rounded on its own: pixel_ray<float> is the order tests/golden/raygen.npz pins, pixel_ray<double>
// the same chain in float64 (the scene sensor).  That holds only in a unit built with -ffp-contract=off, where the compiler fuses no
// multiply with an add; march.hip, localize.hip and sensor.hip, the units that call it, all are.  The one fused chain of the fp32 ray, the
// squared norm in normalize_ray, is spelled with __builtin_fmaf and so is the same under either setting.
//
// The targets (habitat_to_data.py:229-232), element p of the dataset's storage in either layout: colours u8, depths f32 or f16, labels i64
// or u8.  A colour is (float)u8 / 255.0f, one correctly rounded division.
//
// The loss (pipeline.py:506-511): smooth_l1 with beta = 1 on the three colours and on the depth, cross-entropy on the C logits, each summed by
// the caller (train step: float, pose refinement: double) and scaled to a mean there; ray_loss_planes and ray_loss_sem hand the ray's terms
// over unscaled and write its gradients scaled, g * scale * inv_n from left to right.
#pragma once
#include <cmath>
#include <cstdint>

#include <hip/hip_runtime.h>

namespace mnf {

// ---------------------------------------------------------------------------------------------------------------- ray
// d: the un-normalised direction; cam0, cam1: handed back for the sensor's ray-depth factor sqrt((cam0 cam0 + cam1 cam1) + 1)
template <typename T>
__device__ __forceinline__ void pixel_ray(int64_t x, int64_t y, int W, int H, T focal, const T *m, T &cam0, T &cam1, T (&d)[3]) {
    const T cx = (T)W * (T)0.5, cy = (T)H * (T)0.5;
    cam0 = ((T)x - cx + (T)0.5) / focal;
    cam1 = ((T)y - cy + (T)0.5) / focal * (T)-1.0;
    const T cam2 = (T)-1.0;
#pragma unroll
    for (int i = 0; i < 3; ++i) d[i] = (cam0 * m[4 * i] + cam1 * m[4 * i + 1]) + cam2 * m[4 * i + 2];
}

// d / |d| in fp32: the squared norm is the fused chain fma(dz, dz, fma(dy, dy, dx dx)), then one square root and three divisions
__device__ __forceinline__ void normalize_ray(float (&d)[3]) {
    const float n = sqrtf(__builtin_fmaf(d[2], d[2], __builtin_fmaf(d[1], d[1], d[0] * d[0])));
    d[0] /= n; d[1] /= n; d[2] /= n;
}

// ---------------------------------------------------------------------------------------------------------------- targets
__device__ __forceinline__ float unit_u8(uint8_t b) { return (float)b / 255.0f; }

__device__ __forceinline__ float load_depth(const void *depths, int f16, int64_t p) {
    return f16 ? (float)reinterpret_cast<const _Float16 *>(depths)[p] : reinterpret_cast<const float *>(depths)[p];
}

__device__ __forceinline__ int64_t load_label(const void *sems, int u8, int64_t p) {
    return u8 ? (int64_t)reinterpret_cast<const uint8_t *>(sems)[p] : reinterpret_cast<const int64_t *>(sems)[p];
}

// ---------------------------------------------------------------------------------------------------------------- loss
__device__ __forceinline__ void smooth_l1(float x, float &val, float &grad) {      // beta = 1
    const float ax = fabsf(x);
    val = ax < 1.0f ? 0.5f * x * x : ax - 0.5f;
    grad = x < -1.0f ? -1.0f : (x > 1.0f ? 1.0f : x);      // torch's branch order: a NaN difference gives a NaN gradient (the guard of pipeline.py:520-529 then drops the step)
}

// A ray's terms and plane gradients come in two halves, colours with depth and the logits, so that a caller without classes can leave the
// second out.  Both work on ray i of the planes of all rays and write a gradient as g * scale * inv_n, or 0 where `zero` is set (the caller
// has given up on the rays this one belongs to).

// rgb, t_rgb, g_rgb [., 3], depth, t_dep, g_dep [.]: the smooth_l1 of each colour is added to the caller's sum l_rgb (float or double), one after
// the other; the depth's is returned
template <typename Idx, typename Acc>
__device__ __forceinline__ float ray_loss_planes(Idx i, const float *rgb, const float *depth, const float *t_rgb, const float *t_dep, float k_rgb,
                                                 float k_dep, float inv_n, bool zero, float *g_rgb, float *g_dep, Acc &l_rgb) {
    float v, g;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        smooth_l1(rgb[3 * i + k] - t_rgb[3 * i + k], v, g);
        l_rgb += (Acc)v;
        g_rgb[3 * i + k] = zero ? 0.0f : g * k_rgb * inv_n;
    }
    smooth_l1(depth[i] - t_dep[i], v, g);
    g_dep[i] = zero ? 0.0f : g * k_dep * inv_n;
    return v;
}

// sem, g_sem [., C], t_lab [.]: the ray's cross-entropy.  A ray whose label lies outside [0, C) contributes 0, reads nothing past its row and
// gets zero gradients; on_bad_label() is called for it, where the caller flags it.
template <typename Idx, typename OnBadLabel>
__device__ __forceinline__ float ray_loss_sem(Idx i, int C, const float *sem, const int64_t *t_lab, float k_sem, float inv_n, bool zero, float *g_sem,
                                              OnBadLabel on_bad_label) {
    const float *lg = sem + (int64_t)i * C;
    float mx = -INFINITY;
    for (int k = 0; k < C; ++k) mx = fmaxf(mx, lg[k]);
    float den = 0.f;
    for (int k = 0; k < C; ++k) den += expf(lg[k] - mx);
    const int64_t lab = t_lab[i];
    const bool lab_ok = lab >= 0 && lab < C;
    if (!lab_ok) on_bad_label();
    const float ce = lab_ok ? logf(den) - (lg[lab] - mx) : 0.0f;
    const bool zero_sem = zero || !lab_ok;
    for (int k = 0; k < C; ++k) g_sem[(int64_t)i * C + k] = zero_sem ? 0.0f : (expf(lg[k] - mx) / den - (k == lab ? 1.0f : 0.0f)) * k_sem * inv_n;
    return ce;
}

}  // namespace mnf
