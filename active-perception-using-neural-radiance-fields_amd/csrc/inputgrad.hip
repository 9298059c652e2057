// Gradients of the radiance field with respect to its INPUTS: what tiny-cuda-nn returns as dL/d(input) of its encodings and
// networks behind `loss.backward()` (scripts/pipeline.py:518; call sites perception/models/radiance_fields/ngp.py:123-169).
//
//   field_input_grad_kernel   per sample, from what the backward (train.hip) left in the train workspace:
//                             dL/d(position) = trilinear derivative of the 16 hash levels applied to dX, and (optional)
//                             dL/d(direction) = W1_head[:, 0:16]^T dZr1 through the closed-form Jacobian of the degree-4 SH.
//   ray_input_grad_kernel     per ray, packed samples grouped by ray: g_o = sum d_pos, g_d = sum (t_mid * d_pos + d_dir).
//
// Both only read their inputs: no atomics, no cross-workgroup sums, the same inputs give the same bits.
#include "field_dev.h"

MNF_DT_BEGIN

struct InputGradArgs {
    const tab4 *table;
    const LevelMeta *levels;      // [16] device (behind the handle's fragments)
    const float *xn;              // [n][3] aabb-normalised positions (normalize_kernel)
    const float *dX;              // [16][Np][4] un-scaled feature gradients (dgrad_kernel)
    int64_t Np, n;
    const half_t *act;            // [tiles][rows][64]
    int32_t rows, row_dZr1, Wh;
    const half_t *frags;          // the handle's 16-bit weights
    const int32_t *sh_slot;       // [Wh][16] slot of W1_head[j][k] in frags
    const float *dirs;            // [n][3], only read with d_dir
    float inv_scale;              // 1 / loss_scale
    float inv_extent[3];          // 1 / (aabb_max - aabb_min)
    float *d_pos, *d_dir;         // [n][3] each, either may be NULL
};

constexpr int kGradThreads = 256;     // one lane = one sample, a wave = one 64-sample tile of the workspace
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

__global__ void __launch_bounds__(kGradThreads) field_input_grad_kernel(const InputGradArgs args) {
    __shared__ float s_w[kMaxHeadWidth * 16];      // W1_head[j][k], k < 16: every lane reads the same word (broadcast)
    const bool want_dir = args.d_dir != nullptr;   // uniform
    if (want_dir) {
        for (int i = threadIdx.x; i < args.Wh * 16; i += kGradThreads) {
            const int32_t s = args.sh_slot[i];
            s_w[i] = s >= 0 ? (float)args.frags[s] : 0.0f;
        }
        __syncthreads();
    }
    const int64_t col = (int64_t)blockIdx.x * kGradThreads + threadIdx.x;
    if (col - (threadIdx.x & 63) >= args.n) return;              // a wave without a sample (wave-uniform)
    const bool valid = col < args.n;
    const int64_t i = valid ? col : args.n - 1;                  // lanes past the end shadow the last sample and store nothing

    if (args.d_pos) {
        float xn[3];
#pragma unroll
        for (int d = 0; d < 3; ++d) xn[d] = args.xn[3 * i + d];
        const bool inside = xn[0] > 0.0f && xn[0] < 1.0f && xn[1] > 0.0f && xn[1] < 1.0f && xn[2] > 0.0f && xn[2] < 1.0f;
        const bool in_box = __ballot(!inside) == 0ull;           // wave-uniform: the cheap dense-level wrap applies (as the forward)
        const LevelsPtr lv = levels_here(args.levels);
        const float4 *gsrc = reinterpret_cast<const float4 *>(args.dX) + i;
        float acc[3] = {0.f, 0.f, 0.f};
        // the forward's gathers, double-buffered as its prep[q] groups: kGradLevels levels per group, the next group's loads are issued before this one's
        // are consumed, so up to 2 x 8 x kGradLevels gathers are in flight per lane
        LevelPrep prep[2][kGradLevels];
        tab4 v[2][kGradLevels][8];
        float4 g[2][kGradLevels];
#pragma unroll
        for (int q = 0; q < kGradLevels; ++q) {
            hash_prep(level_meta(lv, q), xn, prep[0][q], in_box);
            hash_load(args.table, prep[0][q], v[0][q]);
            g[0][q] = gsrc[(int64_t)q * args.Np];
        }
#pragma unroll
        for (int kb = 0; kb < 16 / kGradLevels; ++kb) {
            const int cur = kb & 1, nxt = cur ^ 1;
            if (kb + 1 < 16 / kGradLevels) {
#pragma unroll
                for (int q = 0; q < kGradLevels; ++q) {
                    const int l = kGradLevels * (kb + 1) + q;
                    hash_prep(level_meta(lv, l), xn, prep[nxt][q], in_box);
                    hash_load(args.table, prep[nxt][q], v[nxt][q]);
                    g[nxt][q] = gsrc[(int64_t)l * args.Np];
                }
            }
#pragma unroll
            for (int q = 0; q < kGradLevels; ++q) level_grad(level_meta(lv, kGradLevels * kb + q), xn, prep[cur][q], v[cur][q], g[cur][q], acc);
            // pin the group's arithmetic here: left free, the compiler sinks all 16 levels' sums behind the last gather and keeps every entry live
            asm volatile("" : "+v"(acc[0]), "+v"(acc[1]), "+v"(acc[2]));
            __builtin_amdgcn_sched_barrier(0);
        }
        if (valid) {
#pragma unroll
            for (int d = 0; d < 3; ++d) args.d_pos[3 * i + d] = acc[d] * args.inv_extent[d];      // xn = (pos - aabb_min) / (aabb_max - aabb_min)
        }
    }

    if (want_dir) {
        // dL/dSH[k] = (1 / loss_scale) sum_j W1[j][k] dZr1[j][sample]; row j of the tile is 64 consecutive 16-bit values (one per lane)
        const half_t *dz = args.act + ((col >> 6) * args.rows + args.row_dZr1) * 64 + (threadIdx.x & 63);
        float s[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) s[k] = 0.0f;
        for (int j0 = 0; j0 < args.Wh; j0 += 8) {
            float z[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) z[j] = (float)dz[(int64_t)(j0 + j) * 64];
#pragma unroll
            for (int j = 0; j < 8; ++j)
#pragma unroll
                for (int k = 1; k < 16; ++k) s[k] = __builtin_fmaf(s_w[(j0 + j) * 16 + k], z[j], s[k]);      // (k = 0: the constant harmonic)
        }
        if (valid) {
            // the forward's argument (field_dev.h sh4): 2u - 1 with u = (d + 1) / 2, chain factor 1
            const float x = ((args.dirs[3 * i] + 1.0f) / 2.0f) * 2.0f - 1.0f;
            const float y = ((args.dirs[3 * i + 1] + 1.0f) / 2.0f) * 2.0f - 1.0f;
            const float z = ((args.dirs[3 * i + 2] + 1.0f) / 2.0f) * 2.0f - 1.0f;
            const float x2 = x * x, y2 = y * y, z2 = z * z;
            constexpr float c1 = 0.48860251190291987f, c2 = 1.0925484305920792f, c3 = 0.94617469575755997f, c5 = 0.54627421529603959f,
                            c6 = 0.59004358992664352f, c7 = 2.8906114426405538f, c8 = 0.45704579946446572f, c9 = 0.3731763325901154f,
                            c10 = 1.4453057213202769f;
            // Jacobian of the 16 polynomials of sh4, column by column
            const float gx = -c1 * s[3] + c2 * y * s[4] - c2 * z * s[7] + 2.0f * c5 * x * s[8] - 6.0f * c6 * x * y * s[9] + c7 * y * z * s[10]
                             + c8 * (1.0f - 5.0f * z2) * s[13] + 2.0f * c10 * x * z * s[14] + 3.0f * c6 * (y2 - x2) * s[15];
            const float gy = -c1 * s[1] + c2 * x * s[4] - c2 * z * s[5] - 2.0f * c5 * y * s[8] + 3.0f * c6 * (y2 - x2) * s[9] + c7 * x * z * s[10]
                             + c8 * (1.0f - 5.0f * z2) * s[11] - 2.0f * c10 * y * z * s[14] + 6.0f * c6 * x * y * s[15];
            const float gz = c1 * s[2] - c2 * y * s[5] + 2.0f * c3 * z * s[6] - c2 * x * s[7] + c7 * x * y * s[10] - 10.0f * c8 * y * z * s[11]
                             + c9 * (15.0f * z2 - 3.0f) * s[12] - 10.0f * c8 * x * z * s[13] + c10 * (x2 - y2) * s[14];
            args.d_dir[3 * i] = gx * args.inv_scale;
            args.d_dir[3 * i + 1] = gy * args.inv_scale;
            args.d_dir[3 * i + 2] = gz * args.inv_scale;
        }
    }
}

int field_input_grad_impl(mnf_field_t f, const InputGradView &view, const float *directions, int64_t n, float loss_scale, float *d_positions,
                          float *d_directions, hipStream_t stream) {
    InputGradArgs a;
    a.table = reinterpret_cast<const tab4 *>(f->d_table);
    a.levels = reinterpret_cast<const LevelMeta *>(reinterpret_cast<const char *>(f->d_frags) + (size_t)f->shape.blocks_total * 1024);
    a.xn = view.xn; a.dX = view.dX; a.Np = view.Np; a.n = n;
    a.act = reinterpret_cast<const half_t *>(view.act); a.rows = view.rows; a.row_dZr1 = view.row_dZr1; a.Wh = f->cfg.neurons / 2;
    a.frags = reinterpret_cast<const half_t *>(f->d_frags); a.sh_slot = view.sh_slot;
    a.dirs = directions; a.inv_scale = 1.0f / loss_scale;
    for (int d = 0; d < 3; ++d) a.inv_extent[d] = 1.0f / (f->cfg.aabb[3 + d] - f->cfg.aabb[d]);
    a.d_pos = d_positions; a.d_dir = d_directions;
    MNF_REQUIRE(a.Wh <= kMaxHeadWidth, "field_backward_inputs: unsupported width");
    {
        ProfScope ps("field_input_grad", stream);
        hipLaunchKernelGGL(field_input_grad_kernel, dim3((unsigned)ceil_div(n, kGradThreads)), dim3(kGradThreads), 0, stream, a);
    }
    return launch_status("field_input_grad_kernel");
}

MNF_DT_END

#ifndef MNF_BF16   // ---- operand-type independent: compiled once
namespace mnf {

// One wave per ray.  Lane L adds the ray's samples L, L + 64, L + 128, ... in index order; the 64 partial sums are then added by a fixed
// butterfly (lane ^ 32, ^ 16, ... ^ 1: every lane ends with the same bits).  The order depends on nothing but the ray's sample count.
__global__ void __launch_bounds__(256) ray_input_grad_kernel(const float *__restrict__ d_pos, const float *__restrict__ d_dir,
                                                             const float *__restrict__ t_starts, const float *__restrict__ t_ends,
                                                             const int64_t *__restrict__ chunk_starts, const int64_t *__restrict__ chunk_cnts,
                                                             int32_t n_rays, int64_t n_samples, float *__restrict__ g_o, float *__restrict__ g_d) {
    const int lane = threadIdx.x & 63;
    const int64_t ray = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (ray >= n_rays) return;
    int64_t s0 = chunk_starts[ray], cnt = chunk_cnts[ray];
    if (s0 < 0 || cnt < 0) { s0 = 0; cnt = 0; }
    const int64_t s1 = s0 + cnt < n_samples ? s0 + cnt : n_samples;      // never past the arrays, whatever the chunks say
    float so[3] = {0.f, 0.f, 0.f}, sd[3] = {0.f, 0.f, 0.f};
    for (int64_t s = s0 + lane; s < s1; s += 64) {
        const float tm = (t_starts[s] + t_ends[s]) / 2.0f;
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            const float p = d_pos[3 * s + d];
            so[d] += p;
            sd[d] += d_dir ? __builtin_fmaf(tm, p, d_dir[3 * s + d]) : tm * p;
        }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1)
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            so[d] += __shfl_xor(so[d], m, 64);
            sd[d] += __shfl_xor(sd[d], m, 64);
        }
    if (lane < 3) {
        if (g_o) g_o[3 * ray + lane] = lane == 0 ? so[0] : (lane == 1 ? so[1] : so[2]);
        if (g_d) g_d[3 * ray + lane] = lane == 0 ? sd[0] : (lane == 1 ? sd[1] : sd[2]);
    }
}

}  // namespace mnf

using namespace mnf;

extern "C" int mnf_field_backward_inputs(mnf_field_t f, const float *positions, const float *directions, int64_t n, void *workspace,
                                         int64_t workspace_bytes, float loss_scale, float *d_positions, float *d_directions, mnf_stream_t stream) {
    (void)positions;      // the workspace holds them normalised, as the backward's scatter read them
    MNF_REQUIRE(f, "field_backward_inputs: null handle");
    MNF_REQUIRE(d_positions || d_directions, "field_backward_inputs: no output asked for");
    MNF_REQUIRE(n >= 0 && loss_scale > 0.f, "field_backward_inputs: bad arguments");
    MNF_REQUIRE(!d_directions || directions || n == 0, "field_backward_inputs: d_directions needs directions");
    if (n == 0) return MNF_OK;
    const int64_t need = mnf_field_train_workspace_bytes(f, n);
    MNF_REQUIRE(need >= 0, "field_backward_inputs: unsupported shape");
    if (!workspace || workspace_bytes < need) {
        set_error("field_backward_inputs: workspace too small (%lld < %lld bytes)", (long long)workspace_bytes, (long long)need);
        return MNF_ERR_WORKSPACE;
    }
    InputGradView view;
    const int rc = f->cfg.mfma_bf16 ? bf16::input_grad_view_impl(f, workspace, n, view) : f16::input_grad_view_impl(f, workspace, n, view);
    if (rc) return rc;
    return f->cfg.mfma_bf16 ? bf16::field_input_grad_impl(f, view, directions, n, loss_scale, d_positions, d_directions, as_stream(stream))
                            : f16::field_input_grad_impl(f, view, directions, n, loss_scale, d_positions, d_directions, as_stream(stream));
}

extern "C" int mnf_ray_input_gradients(const float *d_positions, const float *d_directions, const float *t_starts, const float *t_ends,
                                       const int64_t *chunk_starts, const int64_t *chunk_cnts, int32_t n_rays, int64_t n_samples, float *g_rays_o,
                                       float *g_rays_d, mnf_stream_t stream) {
    MNF_REQUIRE(n_rays >= 0 && n_samples >= 0, "ray_input_gradients: negative count");
    MNF_REQUIRE(g_rays_o || g_rays_d, "ray_input_gradients: no output asked for");
    if (n_rays == 0) return MNF_OK;
    MNF_REQUIRE(chunk_starts && chunk_cnts, "ray_input_gradients: null chunk arrays");
    MNF_REQUIRE(n_samples == 0 || (d_positions && t_starts && t_ends), "ray_input_gradients: null pointer");
    hipLaunchKernelGGL(ray_input_grad_kernel, dim3((unsigned)ceil_div(n_rays, 4)), dim3(256), 0, as_stream(stream), d_positions, d_directions, t_starts,
                       t_ends, chunk_starts, chunk_cnts, n_rays, n_samples, g_rays_o, g_rays_d);
    return launch_status("ray_input_grad_kernel");
}
#endif  // MNF_BF16
