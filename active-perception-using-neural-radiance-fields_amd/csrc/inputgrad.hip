// Gradients of the radiance field with respect to its INPUTS: what tiny-cuda-nn returns as dL/d(input) of its encodings and
// networks behind `loss.backward()` (scripts/pipeline.py:518; call sites perception/models/radiance_fields/ngp.py:123-169).
//
//   field_input_grad_kernel   per sample, from what the backward (train.hip) left in the train workspace:
//                             dL/d(position) = trilinear derivative of the 16 hash levels applied to dX, and (optional)
//                             dL/d(direction) = W1_head[:, 0:16]^T dZr1 through the closed-form Jacobian of the degree-4 SH.
//   ray_input_grad_kernel     per ray, packed samples grouped by ray: g_o = sum d_pos, g_d = sum (t_mid * d_pos + d_dir).
//   train_render_ray_grad_kernel   the two as one launch for the fused train render: from the step's workspace to g_o / g_d, one wave per ray.
//
// All only read their inputs: no atomics, no cross-workgroup sums, the same inputs give the same bits.
#include "inputgrad_dev.h"

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
            float gx, gy, gz;
            sh4_jacobian_t(args.dirs + 3 * i, s, gx, gy, gz);
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

// ---- the two kernels above as one, for the fused train render (trainstep.hip: mnf_train_render_backward_rays): from the step's workspace straight to the
// per-ray sums, no per-sample array in between.
// field_input_grad_kernel's two loops as functions.  (That kernel keeps them written out: called through these its register allocation changes, 234 -> 243
// VGPRs, and its instruction stream is pinned.)
// acc += sum over the 16 levels of level_grad, for the lane's sample at xn with its feature gradients at gsrc[level * Np] (dX, [16][Np][4]).
// The forward's gathers, double-buffered as its prep[q] groups: kGradLevels levels per group, the next group's loads are issued before this one's
// are consumed, so up to 2 x 8 x kGradLevels gathers are in flight per lane.  `in_box` is wave-uniform (hash_prep).
__device__ __forceinline__ void levels_grad(const tab4 *table, const LevelsPtr lv, const float4 *gsrc, int64_t Np, const float xn[3], bool in_box,
                                            float (&acc)[3]) {
    LevelPrep prep[2][kGradLevels];
    tab4 v[2][kGradLevels][8];
    float4 g[2][kGradLevels];
#pragma unroll
    for (int q = 0; q < kGradLevels; ++q) {
        hash_prep(level_meta(lv, q), xn, prep[0][q], in_box);
        hash_load(table, prep[0][q], v[0][q]);
        g[0][q] = gsrc[(int64_t)q * Np];
    }
#pragma unroll
    for (int kb = 0; kb < 16 / kGradLevels; ++kb) {
        const int cur = kb & 1, nxt = cur ^ 1;
        if (kb + 1 < 16 / kGradLevels) {
#pragma unroll
            for (int q = 0; q < kGradLevels; ++q) {
                const int l = kGradLevels * (kb + 1) + q;
                hash_prep(level_meta(lv, l), xn, prep[nxt][q], in_box);
                hash_load(table, prep[nxt][q], v[nxt][q]);
                g[nxt][q] = gsrc[(int64_t)l * Np];
            }
        }
#pragma unroll
        for (int q = 0; q < kGradLevels; ++q) level_grad(level_meta(lv, kGradLevels * kb + q), xn, prep[cur][q], v[cur][q], g[cur][q], acc);
        // pin the group's arithmetic here: left free, the compiler sinks all 16 levels' sums behind the last gather and keeps every entry live
        asm volatile("" : "+v"(acc[0]), "+v"(acc[1]), "+v"(acc[2]));
        __builtin_amdgcn_sched_barrier(0);
    }
}

// s[k] += sum_j W1_head[j][k] dZr1[j] of the lane's sample for the 15 non-constant harmonics (k = 0: the constant one); `dz`: the sample's column in
// row row_dZr1 of its activation tile (row j of the tile is 64 consecutive 16-bit values, one per lane), `s_w`: W1_head[j][k], k < 16, in LDS (every
// lane reads the same word: broadcast)
__device__ __forceinline__ void head_sh_sums(const half_t *dz, const float *s_w, int Wh, float (&s)[16]) {
    for (int j0 = 0; j0 < Wh; j0 += 8) {
        float z[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) z[j] = (float)dz[(int64_t)(j0 + j) * 64];
#pragma unroll
        for (int j = 0; j < 8; ++j)
#pragma unroll
            for (int k = 1; k < 16; ++k) s[k] = __builtin_fmaf(s_w[(j0 + j) * 16 + k], z[j], s[k]);
    }
}

struct RayGradArgs {
    const tab4 *table;
    const LevelMeta *levels;
    const float *xn;              // [n][3] the kept samples' aabb-normalised positions (FieldIO::xn_out)
    const float *dX;              // [16][Np][4]
    int64_t Np, n;                // n: the arrays' bound (max_kept)
    const half_t *act;
    int32_t rows, row_dZr1, Wh;
    const half_t *frags;
    const int32_t *sh_slot;
    const float *t_starts, *t_ends;                   // [n] kept
    const int64_t *kept_starts, *kept_cnts;           // [n_rays] the rays' runs
    const int64_t *n_dev;         // the surviving count the backward worked on (a cleared count: dX is stale, nothing is summed)
    const int32_t *skip;          // the step's skip flag (raised: zeros)
    const float *rays_d;          // [n_rays][3], only read with g_d
    int32_t n_rays;
    float inv_scale;
    float inv_extent[3];
    float *g_o, *g_d;             // [n_rays][3] each, either may be NULL
};

constexpr int kRayGradThreads = 256;  // four rays per workgroup

// One wave per ray (ray_input_grad_kernel's shape).  Lane L takes the ray's kept samples L, L + 64, ... in index order: field_input_grad_kernel's position
// gradient of each, added to the lane's partial sums of d_pos and t_mid d_pos; then, for g_d, the lane's partial sums of the 15 non-constant
// s[k] = sum_j W1_head[j][k] dZr1[j] (a second pass: the 15 sums are not live beside the gathers).  A fixed butterfly (lane ^ 32, ^ 16, ... ^ 1) adds the 64
// partial sums, and the SH Jacobian — linear in s, and every sample of a ray shares the ray's direction — is applied once per ray.  No atomics; the order of
// every sum depends on nothing but the ray's sample count.
__global__ void __launch_bounds__(kRayGradThreads) train_render_ray_grad_kernel(const RayGradArgs args) {
    __shared__ float s_w[kMaxHeadWidth * 16];
    const bool want_dir = args.g_d != nullptr;     // uniform
    if (want_dir) {
        for (int i = threadIdx.x; i < args.Wh * 16; i += kRayGradThreads) {
            const int32_t s = args.sh_slot[i];
            s_w[i] = s >= 0 ? (float)args.frags[s] : 0.0f;
        }
        __syncthreads();
    }
    const int lane = threadIdx.x & 63;
    const int64_t ray = (int64_t)blockIdx.x * (kRayGradThreads / 64) + (threadIdx.x >> 6);
    if (ray >= args.n_rays) return;
    int64_t s0 = args.kept_starts[ray], cnt = args.kept_cnts[ray];
    if (s0 < 0 || cnt < 0) { s0 = 0; cnt = 0; }
    int64_t lim = args.n_dev[0] < args.n ? args.n_dev[0] : args.n;      // never past the arrays, and never into what the backward did not write
    if (args.skip[0] > 0) lim = 0;
    const int64_t s1 = s0 + cnt < lim ? s0 + cnt : lim;
    const int c = __builtin_amdgcn_readfirstlane(s1 > s0 ? (int)(s1 - s0) : 0);      // the ray's samples that count (wave-uniform)

    float so[3] = {0.f, 0.f, 0.f}, sd[3] = {0.f, 0.f, 0.f};
    for (int base = 0; base < c; base += 64) {
        const bool valid = base + lane < c;
        const int64_t i = s0 + (valid ? base + lane : c - 1);            // lanes past the run shadow its last sample and add nothing
        float xn[3];
#pragma unroll
        for (int d = 0; d < 3; ++d) xn[d] = args.xn[3 * i + d];
        const bool inside = xn[0] > 0.0f && xn[0] < 1.0f && xn[1] > 0.0f && xn[1] < 1.0f && xn[2] > 0.0f && xn[2] < 1.0f;
        const bool in_box = __ballot(!inside) == 0ull;
        const LevelsPtr lv = levels_here(args.levels);
        float acc[3] = {0.f, 0.f, 0.f};
        levels_grad(args.table, lv, reinterpret_cast<const float4 *>(args.dX) + i, args.Np, xn, in_box, acc);
        const float tm = (args.t_starts[i] + args.t_ends[i]) / 2.0f;
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            const float p = valid ? acc[d] * args.inv_extent[d] : 0.0f;
            so[d] += p;
            sd[d] = __builtin_fmaf(tm, p, sd[d]);
        }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1)
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            so[d] += __shfl_xor(so[d], m, 64);
            sd[d] += __shfl_xor(sd[d], m, 64);
        }
    if (args.g_o && lane < 3) args.g_o[3 * ray + lane] = lane == 0 ? so[0] : (lane == 1 ? so[1] : so[2]);
    if (!want_dir) return;

    float s[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) s[k] = 0.0f;
    for (int base = lane; base < c; base += 64) {
        const int64_t i = s0 + base;
        head_sh_sums(args.act + ((i >> 6) * args.rows + args.row_dZr1) * 64 + (i & 63), s_w, args.Wh, s);
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1)
#pragma unroll
        for (int k = 1; k < 16; ++k) s[k] += __shfl_xor(s[k], m, 64);
    float gx, gy, gz;
    sh4_jacobian_t(args.rays_d + 3 * ray, s, gx, gy, gz);
    if (lane < 3) args.g_d[3 * ray + lane] = lane == 0 ? sd[0] + gx * args.inv_scale : (lane == 1 ? sd[1] + gy * args.inv_scale : sd[2] + gz * args.inv_scale);
}

int train_render_ray_grad_impl(mnf_field_t f, void *field_ws, const RayGradIO &io, hipStream_t stream) {
    InputGradView view;
    const int rc = input_grad_view_impl(f, field_ws, io.n, view);
    if (rc) return rc;
    RayGradArgs a;
    a.table = reinterpret_cast<const tab4 *>(f->d_table);
    a.levels = reinterpret_cast<const LevelMeta *>(reinterpret_cast<const char *>(f->d_frags) + (size_t)f->shape.blocks_total * 1024);
    a.xn = io.xn; a.dX = view.dX; a.Np = view.Np; a.n = io.n;
    a.act = reinterpret_cast<const half_t *>(view.act); a.rows = view.rows; a.row_dZr1 = view.row_dZr1; a.Wh = f->cfg.neurons / 2;
    a.frags = reinterpret_cast<const half_t *>(f->d_frags); a.sh_slot = view.sh_slot;
    a.t_starts = io.t_starts; a.t_ends = io.t_ends; a.kept_starts = io.kept_starts; a.kept_cnts = io.kept_cnts; a.n_dev = io.n_dev; a.skip = io.skip;
    a.rays_d = io.rays_d; a.n_rays = io.n_rays; a.inv_scale = 1.0f / io.loss_scale;
    for (int d = 0; d < 3; ++d) a.inv_extent[d] = 1.0f / (f->cfg.aabb[3 + d] - f->cfg.aabb[d]);
    a.g_o = io.g_o; a.g_d = io.g_d;
    MNF_REQUIRE(a.Wh <= kMaxHeadWidth, "train_render_backward_rays: unsupported width");
    {
        ProfScope ps("train_render_ray_grad", stream);
        hipLaunchKernelGGL(train_render_ray_grad_kernel, dim3((unsigned)ceil_div(io.n_rays, kRayGradThreads / 64)), dim3(kRayGradThreads), 0, stream, a);
    }
    return launch_status("train_render_ray_grad_kernel");
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

int train_render_ray_grad(mnf_field_t f, void *field_ws, const RayGradIO &io, hipStream_t stream) {
    return f->cfg.mfma_bf16 ? bf16::train_render_ray_grad_impl(f, field_ws, io, stream) : f16::train_render_ray_grad_impl(f, field_ws, io, stream);
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
