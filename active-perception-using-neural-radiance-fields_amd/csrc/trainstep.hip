// One training iteration's forward + loss + backward as ONE C call.
//
//   mnf_train_step    scripts/pipeline.py:472-518 for one model: `render_image_with_occgrid_with_depth_guide`
//                     (perception/models/utils.py:63-219: occupancy sampling with the density pre-pass and the visibility
//                     filter of nerfacc/estimators/occ_grid.py:80-238, then `sem_rendering`, utils.py:362-461), the three-term
//                     loss (pipeline.py:506-511) and `loss.backward()` down to the three flat parameter-gradient vectors.
//                     The optimizer step and the NaN guard stay with the caller (pipeline.py:520-532), as does the occupancy
//                     refresh (mnf_update_occupancy).
//   mnf_train_render_forward / mnf_train_render_backward
//                     the same step cut at its loss: pipeline.py:472-489 now, `loss.backward()` (pipeline.py:518) later with whatever gradients the caller's own
//                     loss produced for the four rendered planes.  Same kernels in the same order on either side of the cut (step_forward / step_backward).
//
// All of them are compositions of the library's own entry points plus the small kernels below (stratified near planes, visibility
// filter with compaction, loss + its gradient).  mnf_train_step never synchronises with the host: the marched and the
// surviving sample counts stay on the device (every launch is sized for the caller's upper bounds and reads the actual
// count from device memory), overflow of a bound is detected on the device (the step then yields zero gradients and a
// raised skip flag, which `mnf_adam_step_guarded` honours) and reported through `counts_dev`, which the caller reads
// whenever it wants to (the reference's boolean-mask indexing synchronises twice per step at these points).
//
// Build with -ffp-contract=off (the marcher's near planes feed bit-exact t values).
#include <cmath>
#include <cstddef>

#include "field.h"
#include "philox_dev.h"
#include "pixel_dev.h"
#include "reduce_dev.h"
#include "workspace.h"

// mnf_train_presample's handle: what was marched, for which rays / options, and the two events that order it
struct mnf_presample_s {
    hipEvent_t ev_ready = nullptr, ev_done = nullptr;
    void *ws = nullptr;
    const float *rays_o = nullptr, *rays_d = nullptr;
    const uint8_t *binaries = nullptr;
    int32_t n_rays = 0, stratified = 0, n_levels = 0, res[3] = {0, 0, 0};
    uint64_t seed = 0;
    float near_plane = 0.f, far_plane = 0.f, step = 0.f, cone = 0.f, alpha_thre = 0.f;
    int64_t max_marched = 0;
    int valid = 0, launched = 0;
};

namespace mnf {
// composite_train.hip: the public entry points with the logits class-major, sems[class * sem_stride + sample] (0: [sample][C])
int composite_train_forward_impl(const int64_t *chunk_starts, const int64_t *chunk_cnts, int32_t n_rays, const float *t_starts, const float *t_ends, const float *sigmas,
                                 const float *rgbs, const float *sems, int64_t sem_stride, int32_t n_classes, int64_t n_samples, const float *bkgd, float *out_rgb,
                                 float *out_acc, float *out_depth, float *out_sem, float *weights, float *trans, float *alphas, mnf_stream_t stream);
int composite_train_backward_impl(const int64_t *chunk_starts, const int64_t *chunk_cnts, int32_t n_rays, const float *t_starts, const float *t_ends, const float *sigmas,
                                  const float *rgbs, const float *sems, int64_t sem_stride, int32_t n_classes, int64_t n_samples, const float *bkgd, const float *weights,
                                  const float *trans, const float *out_acc, const float *out_depth, const float *g_rgb, const float *g_acc, const float *g_depth,
                                  const float *g_sem, float *d_sigmas, float *d_rgbs, float *d_sems, mnf_stream_t stream);
namespace {

// occ_grid.py:181-189: near / far planes, stratified jitter near += U[0,1) * step (Philox counter (ray, 0, 7, 0), key = seed)
// Also the step's small zero-fills (loss terms, counters, skip flag, the two small gradient vectors): five separate memsets were five launches of ~5 us.
// The step's fills: what were seven memsets (losses, counters, skip flag, the three gradient vectors, the pre-pass's density array and its work counter) — launches of ~5 us
// each, the 50 MB one with a ~13 us bubble in front of it.
struct StepFills {
    float *g_base, *g_head, *g_sem, *sigma;
    int64_t n_base, n_head, n_sem, n_sigma;
    int32_t *ray_counter;
    const int64_t *adopt;      // a presampled step: the four counters its march's guard left (status bits != 0: the step is skipped), or NULL
};
__device__ __forceinline__ void fill_zero(float *p, int64_t n, int64_t tid, int64_t threads) {
    if (!p) return;
    const int64_t head = ((16 - (reinterpret_cast<uintptr_t>(p) & 15)) & 15) / 4;      // floats in front of the first 16-byte boundary
    const int64_t h = head < n ? head : n;
    for (int64_t i = tid; i < h; i += threads) p[i] = 0.f;
    float4 *q = reinterpret_cast<float4 *>(p + h);
    const int64_t nq = (n - h) / 4;
    for (int64_t i = tid; i < nq; i += threads) q[i] = float4{0.f, 0.f, 0.f, 0.f};
    for (int64_t i = h + nq * 4 + tid; i < n; i += threads) p[i] = 0.f;
}
__global__ void __launch_bounds__(256) planes_kernel(int32_t n, float near_plane, float far_plane, float step, int32_t stratified, uint32_t s0,
                                                     uint32_t s1, float *__restrict__ nearp, float *__restrict__ farp, float *__restrict__ losses,
                                                     int64_t *__restrict__ counts, int32_t *__restrict__ skip, const StepFills z) {
    const int32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (losses) {      // (NULL: a presample — the planes only; nearp NULL: a presampled step — the zero-fills only)
        if (r < 4) { losses[r] = 0.f; counts[r] = z.adopt ? z.adopt[r] : 0; }
        if (r == 0) { *skip = (z.adopt && z.adopt[3] != 0) ? 1 : 0; if (z.ray_counter) *z.ray_counter = 0; }
        const int64_t threads = (int64_t)gridDim.x * blockDim.x;
        fill_zero(z.g_base, z.n_base, r, threads); fill_zero(z.g_head, z.n_head, r, threads); fill_zero(z.g_sem, z.n_sem, r, threads);
        fill_zero(z.sigma, z.n_sigma, r, threads);
    }
    if (r >= n || !nearp) return;
    float v = near_plane;
    if (stratified) v += unit_float(philox4x32_10({(uint32_t)r, 0u, 7u, 0u}, s0, s1).x) * step;
    nearp[r] = v; farp[r] = far_plane;
}

// mean of occs (occ_grid.py:192: alpha_thre = min(alpha_thre, self.occs.mean())) in double: 128 partial sums, then one wave
__global__ void __launch_bounds__(256) mean_partial_kernel(const float *__restrict__ x, int64_t n, double *__restrict__ part) {
    __shared__ double s[256];
    double acc = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) acc += (double)x[i];
    s[threadIdx.x] = acc;
    __syncthreads();
    for (int d = 128; d >= 1; d >>= 1) { if ((int)threadIdx.x < d) s[threadIdx.x] += s[threadIdx.x + d]; __syncthreads(); }
    if (threadIdx.x == 0) part[blockIdx.x] = s[0];
}

__global__ void __launch_bounds__(64) mean_final_kernel(const double *__restrict__ part, int n_part, int64_t n, float alpha_thre, float *__restrict__ out) {
    double acc = 0.0;
    for (int i = threadIdx.x; i < n_part; i += 64) acc += part[i];
    acc = wave_sum_all(acc);
    if (threadIdx.x == 0) out[0] = fminf(alpha_thre, (float)(acc / (double)n));
}

__global__ void __launch_bounds__(1024) max_kernel(const int64_t *__restrict__ x, int64_t n, int64_t *__restrict__ out) {
    __shared__ long long s[1024];
    long long m = 0;
    for (int64_t i = threadIdx.x; i < n; i += 1024) m = x[i] > m ? x[i] : m;
    s[threadIdx.x] = m;
    __syncthreads();
    for (int d = 512; d >= 1; d >>= 1) { if ((int)threadIdx.x < d && s[threadIdx.x + d] > s[threadIdx.x]) s[threadIdx.x] = s[threadIdx.x + d]; __syncthreads(); }
    if (threadIdx.x == 0) out[0] = s[0];
}

// render_visibility_from_density (volrend.py:424-483) on packed samples, one wave per ray: pass 0 counts the survivors of
// each ray, pass 1 (after the prefix sum of the counts) writes them compacted and grouped by ray.
template <bool WRITE>
__global__ void __launch_bounds__(64) visibility_kernel(int32_t n_rays, const int64_t *__restrict__ starts, const int64_t *__restrict__ cnts,
                                                        const float *__restrict__ ts, const float *__restrict__ te, const float *__restrict__ sig,
                                                        float early_stop_eps, const float *__restrict__ alpha_thre_dev,
                                                        int64_t *__restrict__ kept_cnts, const int64_t *__restrict__ kept_starts,
                                                        float *__restrict__ o_ts, float *__restrict__ o_te, int64_t *__restrict__ o_ray,
                                                        int64_t *__restrict__ o_src /* optional: the marched index of every survivor */) {
    const int lane = threadIdx.x;
    const float alpha_thre = alpha_thre_dev[0];
    for (int32_t r = blockIdx.x; r < n_rays; r += gridDim.x) {
        const int64_t s = starts[r];
        const int c = (int)cnts[r];
        float carry = 0.0f;
        int64_t out = WRITE ? kept_starts[r] : 0;
        int kept = 0;
        for (int base = 0; base < c; base += 64) {
            const bool valid = base + lane < c;
            const int64_t k = s + base + lane;
            const float a = valid ? ts[k] : 0.f, b = valid ? te[k] : 0.f;
            const float sdt = valid ? sig[k] * (b - a) : 0.0f;
            float incl = sdt;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) { const float u = __shfl_up(incl, d, 64); if (lane >= d) incl += u; }
            const float alpha = 1.0f - expf(-sdt);
            const float trans = expf(-((incl - sdt) + carry));
            carry += __shfl(incl, 63, 64);
            bool vis = valid && trans >= early_stop_eps;
            if (alpha_thre > 0.0f) vis = vis && alpha >= alpha_thre;
            const unsigned long long m = __ballot(vis);
            if (WRITE && vis) {
                const int64_t dst = out + __popcll(m & ((1ull << lane) - 1ull));
                o_ts[dst] = a; o_te[dst] = b; o_ray[dst] = r;
                if (o_src) o_src[dst] = k;
            }
            const int nk = __popcll(m);
            out += nk; kept += nk;
        }
        if (!WRITE && lane == 0) kept_cnts[r] = kept;
    }
}

// pipeline.py:506-511: 10 * smooth_l1(rgb, pixels) + smooth_l1(depth, dep[:, None]) / 5 + cross_entropy(sem, labels) / 2 (all
// "mean" reductions) and its gradient with respect to the rendered rgb / depth / semantic logits.  One lane per ray, its terms and gradients from
// pixel_dev.h's two halves.
__global__ void __launch_bounds__(256) loss_kernel(int32_t n_rays, int32_t C, const float *__restrict__ rgb, const float *__restrict__ depth,
                                                   const float *__restrict__ sem, const float *__restrict__ t_rgb, const float *__restrict__ t_dep,
                                                   const int64_t *__restrict__ t_sem, float *__restrict__ g_rgb, float *__restrict__ g_dep,
                                                   float *__restrict__ g_sem, float *__restrict__ losses /* [4]: total, rgb, depth, sem */,
                                                   int64_t *__restrict__ status, int32_t *__restrict__ skip) {
    __shared__ float s_acc[3][4];
    const int32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    float l_rgb = 0.f, l_dep = 0.f, l_sem = 0.f;
    if (r < n_rays) {
        const float inv_r = 1.0f / (float)n_rays;
        l_dep = ray_loss_planes(r, rgb, depth, t_rgb, t_dep, 10.0f / 3.0f, 0.2f, inv_r, false, g_rgb, g_dep, l_rgb);
        // F.cross_entropy raises a device assert for a class id outside [0, C); here the step is flagged (status bit 8, skip
        // raised: no optimizer update) and the ray contributes nothing, instead of reading past the logits row
        l_sem = ray_loss_sem(r, C, sem, t_sem, 0.5f, inv_r, false, g_sem, [&] { atomicOr(reinterpret_cast<unsigned long long *>(status), 8ull); atomicAdd(skip, 1); });
    }
    wave_sum_all_each(l_rgb, l_dep, l_sem);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { s_acc[0][wave] = l_rgb; s_acc[1][wave] = l_dep; s_acc[2][wave] = l_sem; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const float inv_r = 1.0f / (float)n_rays;
        const float a = (s_acc[0][0] + s_acc[0][1] + s_acc[0][2] + s_acc[0][3]) * inv_r / 3.0f;
        const float b = (s_acc[1][0] + s_acc[1][1] + s_acc[1][2] + s_acc[1][3]) * inv_r;
        const float c = (s_acc[2][0] + s_acc[2][1] + s_acc[2][2] + s_acc[2][3]) * inv_r;
        atomicAdd(&losses[1], a); atomicAdd(&losses[2], b); atomicAdd(&losses[3], c);
        atomicAdd(&losses[0], a * 10.0f + b / 5.0f + c / 2.0f);
    }
}

// Device-side bound checks (what the host did between its two syncs in rounds 1-2).  counts_dev: [marched, kept, longest ray, status];
// status bits: 1 marched > max_marched, 2 a ray longer than a scratch row, 4 kept > max_kept, 8 class id out of range, 16 no sample
// survived (the reference `continue`s: no backward, no optimizer step).  On overflow every per-ray count is zeroed, so the kernels
// behind the guard find nothing to do: the step yields zero gradients and `skip` > 0.
__global__ void __launch_bounds__(256) guard_marched_kernel(int32_t n_rays, int64_t *__restrict__ counts, int64_t *__restrict__ starts,
                                                            const int64_t *__restrict__ totals /* [0] marched, [2] longest */, int64_t max_marched,
                                                            int64_t row_cap, int64_t *__restrict__ eff /* [0] */, int64_t *__restrict__ counts_dev,
                                                            int32_t *__restrict__ skip) {
    const int32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t tot = totals[0], longest = totals[2];
    const bool bad = tot > max_marched || longest > row_cap;
    if (bad && r < n_rays) { counts[r] = 0; starts[r] = 0; }
    if (r == 0) {
        eff[0] = bad ? 0 : tot;
        const unsigned long long bits = (unsigned long long)((tot > max_marched ? 1 : 0) | (longest > row_cap ? 2 : 0));
        if (!skip) {      // a presample: its own four counters (the step's planes_kernel adopts them: PreReport)
            counts_dev[0] = tot; counts_dev[1] = 0; counts_dev[2] = longest; counts_dev[3] = (int64_t)bits;
        } else {
            counts_dev[0] = tot; counts_dev[2] = longest;
            if (bad) { atomicOr(reinterpret_cast<unsigned long long *>(counts_dev + 3), bits); atomicAdd(skip, 1); }
        }
    }
}

__global__ void __launch_bounds__(256) guard_kept_kernel(int32_t n_rays, int64_t *__restrict__ kept_cnts, int64_t *__restrict__ kept_starts,
                                                         const int64_t *__restrict__ totals /* [1] kept */, int64_t max_kept,
                                                         int64_t *__restrict__ eff /* [1] */, int64_t *__restrict__ counts_dev, int32_t *__restrict__ skip) {
    const int32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t kept = totals[1];
    const bool bad = kept > max_kept;
    if (bad && r < n_rays) { kept_cnts[r] = 0; kept_starts[r] = 0; }
    if (r == 0) {
        counts_dev[1] = kept;
        eff[1] = bad ? 0 : kept;
        if (bad || kept == 0) {
            atomicOr(reinterpret_cast<unsigned long long *>(counts_dev + 3), bad ? 4ull : 16ull);
            atomicAdd(skip, 1);
        }
    }
}

__global__ void set3_kernel(float *dst, float a, float b, float c) { dst[0] = a; dst[1] = b; dst[2] = c; }

// mnf_train_render_forward's tail: the four per-ray planes from the workspace (where the backward reads the opacity and the depth again) into the caller's
// buffers, the head kernel's block ticket back to 0, and the forward's verdict (a guard fired, or nothing survived) into the word behind the ticket: the backward's
// head reads it there, a word no block of its own launch writes
__global__ void __launch_bounds__(256) outputs_kernel(int64_t n_rays, int32_t C, const float *__restrict__ o_rgb, const float *__restrict__ o_acc,
                                                      const float *__restrict__ o_dep, const float *__restrict__ o_sem, float *__restrict__ rgb,
                                                      float *__restrict__ acc, float *__restrict__ dep, float *__restrict__ sem, const int32_t *__restrict__ skip,
                                                      uint32_t *__restrict__ ticket) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) { ticket[0] = 0u; ticket[1] = *skip > 0 ? 1u : 0u; }
    if (i < n_rays) { acc[i] = o_acc[i]; dep[i] = o_dep[i]; }
    if (i < n_rays * 3) rgb[i] = o_rgb[i];
    if (i < n_rays * C) sem[i] = o_sem[i];
}

// mnf_train_render_backward's head, in planes_kernel's manner (its fills ride on one launch): the three parameter-gradient vectors are zeroed and the caller's
// four output gradients are read through their strides (autograd hands over expanded stride-0 tensors for `x.mean()` and transposed views for other losses)
// into the workspace's dense per-ray arrays.  NULL = zero.  A non-finite incoming value — `loss.backward()` of a NaN loss — is stored as 0 and raises status
// bit 32 and the skip flag; the last block to finish then clears the surviving-sample count the kernels behind it work on, so the step yields zero
// gradients (pipeline.py:520-529 decided on the device).  With the forward's verdict raised (outputs_kernel's word) every array is zeroed (wave-uniform: one word, constant over the launch).
struct GradIn { const float *p; int64_t rs, cs; };      // a [rows, cols] gradient: element (r, c) at p[r * rs + c * cs]
struct GradFills { float *g_base, *g_head, *g_sem; int64_t n_base, n_head, n_sem; };
__device__ __forceinline__ float finite_or_flag(float v, bool &bad) {
    if ((__float_as_uint(v) & 0x7F800000u) != 0x7F800000u) return v;
    bad = true;
    return 0.f;
}
__device__ __forceinline__ bool read_gradient(float *dst, const GradIn g, int64_t rows, int32_t cols, bool dead, int64_t tid, int64_t threads) {
    const int64_t n = rows * cols;
    if (dead || !g.p) { fill_zero(dst, n, tid, threads); return false; }
    bool bad = false;
    const bool dense = cols == 1 ? g.rs == 1 : (g.cs == 1 && g.rs == cols);
    if (dense) {      // 16-byte loads from the source's first 16-byte boundary on, scalar head and tail (fill_zero's shape); `dst` is 256-byte aligned
        const int64_t head = ((16 - (reinterpret_cast<uintptr_t>(g.p) & 15)) & 15) / 4;
        const int64_t h = head < n ? head : n;
        for (int64_t i = tid; i < h; i += threads) dst[i] = finite_or_flag(g.p[i], bad);
        const float4 *q = reinterpret_cast<const float4 *>(g.p + h);
        const int64_t nq = (n - h) / 4;
        for (int64_t i = tid; i < nq; i += threads) {
            const float4 v = q[i];
            const float4 o = float4{finite_or_flag(v.x, bad), finite_or_flag(v.y, bad), finite_or_flag(v.z, bad), finite_or_flag(v.w, bad)};
            float *d = dst + h + i * 4;
            if (h == 0) *reinterpret_cast<float4 *>(d) = o;
            else { d[0] = o.x; d[1] = o.y; d[2] = o.z; d[3] = o.w; }
        }
        for (int64_t i = h + nq * 4 + tid; i < n; i += threads) dst[i] = finite_or_flag(g.p[i], bad);
    } else {
        for (int64_t i = tid; i < n; i += threads) {
            const int64_t r = i / cols, c = i - r * cols;
            dst[i] = finite_or_flag(g.p[r * g.rs + c * g.cs], bad);
        }
    }
    return bad;
}
__global__ void __launch_bounds__(256) gradients_in_kernel(int32_t n_rays, int32_t C, const GradIn i_rgb, const GradIn i_acc, const GradIn i_dep, const GradIn i_sem,
                                                           float *__restrict__ g_rgb, float *__restrict__ g_acc, float *__restrict__ g_dep,
                                                           float *__restrict__ g_sem, const GradFills z, int64_t *counts_dev, int32_t *skip,
                                                           int64_t *eff /* [1]: surviving samples the backward works on */, uint32_t *ticket) {
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, threads = (int64_t)gridDim.x * blockDim.x;
    fill_zero(z.g_base, z.n_base, tid, threads); fill_zero(z.g_head, z.n_head, tid, threads); fill_zero(z.g_sem, z.n_sem, tid, threads);
    const bool dead = ticket[1] != 0u;      // the forward found nothing to render (its verdict as outputs_kernel left it: not the flag blocks of this launch raise)
    bool bad = read_gradient(g_rgb, i_rgb, n_rays, 3, dead, tid, threads);
    bad |= read_gradient(g_acc, i_acc, n_rays, 1, dead, tid, threads);
    bad |= read_gradient(g_dep, i_dep, n_rays, 1, dead, tid, threads);
    bad |= read_gradient(g_sem, i_sem, n_rays, C, dead, tid, threads);
    const int any_bad = __syncthreads_or(bad ? 1 : 0);
    if (threadIdx.x == 0) {
        // (the flag is raised, read and ordered by device-scope atomics only; the fence — a write-back of the L2 the fills have just dirtied — is paid by a
        //  block that raised it, which orders its raise in front of its ticket, and by no other)
        if (any_bad) { atomicOr(reinterpret_cast<unsigned long long *>(counts_dev + 3), 32ull); atomicAdd(skip, 1); __threadfence(); }
        if (atomicAdd(ticket, 1u) == gridDim.x - 1) {      // every other block has raised its flag, if it had to
            if (atomicAdd(skip, 0) > 0) eff[1] = 0;
            ticket[0] = 0u;
        }
    }
}

// The two small blocks of a workspace, word by word.  The asserts pin every position: an adopting step reads a presample's blocks, a render backward the forward's.
struct StepWords {                        // `totals`: 256 int64 words
    int64_t marched, kept, longest, spare3;      // [0..2] the totals of the two scans, and the longest ray (max_kernel)
    int64_t eff[2], spare6;                      // [4..5] marched, kept: the counts the kernels behind the guards work on
    int32_t ray_counter, spare7;          // [7] the pre-pass's work counter
    double mean_part[128], spare136[24];         // [8..135] the occupancy mean's partial sums
    int64_t pre_report[4], spare164[36];         // [160..163] a presample's report: its guard's four counters, which the adopting step's planes_kernel copies
    uint32_t ticket, verdict;             // [200] mnf_train_render_*'s block ticket and, in the 32 bits behind it, the forward's verdict
    int64_t spare201[55];
};
struct StepScalars {                      // `alpha_thre`: 64 floats
    float alpha_thre, spare1[7];          // [0] the visibility filter's threshold (mean_final_kernel)
    float bkgd[3], spare11[5];            // [8..10] a by-value background colour (set3_kernel)
    float render_losses[4], spare20[44];  // [16..19] the loss terms planes_kernel zeroes for a mnf_train_render_forward (nobody reads them)
};
static_assert(sizeof(StepWords) == 2048 && offsetof(StepWords, marched) == 0 && offsetof(StepWords, kept) == 8 && offsetof(StepWords, longest) == 16 &&
              offsetof(StepWords, eff) == 32 && offsetof(StepWords, ray_counter) == 56 && offsetof(StepWords, mean_part) == 64 &&
              offsetof(StepWords, pre_report) == 1280 && offsetof(StepWords, ticket) == 1600 && offsetof(StepWords, verdict) == 1604, "StepWords: a word has moved");
static_assert(sizeof(StepScalars) == 256 && offsetof(StepScalars, alpha_thre) == 0 && offsetof(StepScalars, bkgd) == 32 &&
              offsetof(StepScalars, render_losses) == 64, "StepScalars: a word has moved");

// What the parameter-independent head of a step leaves behind (mnf_train_presample), and the same part of a step's own workspace: the part the march fills.
struct SampleWs {
    float *nearp, *farp, *scratch_ts, *scratch_te;
    StepScalars *scalars; StepWords *words;      // the two small blocks
    int64_t *counts, *starts, *scan;
    float *ts, *te; int64_t *ray;      // the packed samples
    int64_t bytes;                     // of the workspace it was carved from, whole
};

struct StepWs : SampleWs {
    int64_t *kept_cnts, *kept_starts;
    int64_t *kept_scan;                // the step's own scan buffer.  After an adoption `scan` is the presample's; the kept-sample scan never writes there
    float *sigma;                      // marched
    float *k_ts, *k_te, *k_rgb, *k_sigma, *k_sem, *k_pos, *k_w, *k_tr, *k_dsig, *k_drgb, *k_dsem;   // kept
    int64_t *k_ray;
    void *rows; int64_t *k_src;        // the pre-pass's feature rows [max_marched][64] x 16 bit and every surviving sample's row (field_rows_supported)
    float *o_rgb, *o_acc, *o_dep, *o_sem, *g_rgb, *g_dep, *g_sem;   // per ray
    float *g_acc;                      // per ray: the caller's opacity gradient (mnf_train_render_backward; the step's own loss has none)
    void *field_ws;
    int64_t field_ws_bytes;
};

SampleWs carve_sample(void *base, int64_t R, int32_t cap, int64_t max_marched) {
    SampleWs w;
    Carver c(base);
    w.nearp = c.take<float>(R); w.farp = c.take<float>(R); w.scalars = c.take<StepScalars>(1);
    w.counts = c.take<int64_t>(R); w.starts = c.take<int64_t>(R);
    w.words = c.take<StepWords>(1); w.scan = (int64_t *)c.take((size_t)mnf_scan_workspace_bytes(R));
    w.scratch_ts = c.take<float>((size_t)R * cap); w.scratch_te = c.take<float>((size_t)R * cap);
    w.ts = c.take<float>(max_marched); w.te = c.take<float>(max_marched); w.ray = c.take<int64_t>(max_marched);
    w.bytes = c.bytes();
    return w;
}

StepWs carve_step(void *base, mnf_field_t f, int64_t R, int32_t cap, int64_t max_marched, int64_t max_kept) {
    StepWs w;
    Carver c(base);
    const size_t C = f->cfg.num_semantic_classes;
    w.nearp = c.take<float>(R); w.farp = c.take<float>(R); w.scalars = c.take<StepScalars>(1);
    w.counts = c.take<int64_t>(R); w.starts = c.take<int64_t>(R); w.kept_cnts = c.take<int64_t>(R); w.kept_starts = c.take<int64_t>(R);
    w.words = c.take<StepWords>(1); w.kept_scan = w.scan = (int64_t *)c.take((size_t)mnf_scan_workspace_bytes(R));
    w.scratch_ts = c.take<float>((size_t)R * cap); w.scratch_te = c.take<float>((size_t)R * cap);
    w.ts = c.take<float>(max_marched); w.te = c.take<float>(max_marched); w.sigma = c.take<float>(max_marched); w.ray = c.take<int64_t>(max_marched);
    w.k_ts = c.take<float>(max_kept); w.k_te = c.take<float>(max_kept); w.k_ray = c.take<int64_t>(max_kept);
    w.k_rgb = c.take<float>(max_kept * 3); w.k_sigma = c.take<float>(max_kept); w.k_sem = c.take<float>(max_kept * C);
    w.k_pos = c.take<float>(max_kept * 3); w.k_w = c.take<float>(max_kept); w.k_tr = c.take<float>(max_kept);
    w.k_dsig = c.take<float>(max_kept); w.k_drgb = c.take<float>(max_kept * 3); w.k_dsem = c.take<float>(max_kept * C);
    w.o_rgb = c.take<float>(R * 3); w.o_acc = c.take<float>(R); w.o_dep = c.take<float>(R); w.o_sem = c.take<float>(R * C);
    w.g_rgb = c.take<float>(R * 3); w.g_dep = c.take<float>(R); w.g_sem = c.take<float>(R * C);
    w.rows = nullptr; w.k_src = nullptr;
    if (field_rows_supported(f)) { w.rows = c.take((size_t)max_marched * 128); w.k_src = c.take<int64_t>(max_kept); }
    w.field_ws_bytes = mnf_field_train_workspace_bytes(f, max_kept);
    w.field_ws = c.take((size_t)w.field_ws_bytes);
    w.g_acc = c.take<float>(R);      // (behind everything else: every other offset is what it was)
    w.bytes = c.bytes();
    return w;
}

inline int32_t scratch_cap(int32_t n_rays) {
    const int64_t c = ((int64_t)1 << 27) / (n_rays > 0 ? n_rays : 1);
    return (int32_t)(c < 64 ? 64 : (c > 2048 ? 2048 : c));
}

inline int64_t *eff_counts(const SampleWs &w) { return w.words->eff; }      // [0] marched, [1] kept samples the kernels behind the guards work on

// The background both sides of the loss composite over: the caller's device colour, else the by-value one where not black (step_forward leaves it in `w`), else none
inline const float *background(const SampleWs &w, const mnf_train_opts *opts) {
    if (opts->render_bkgd_dev) return opts->render_bkgd_dev;
    return opts->render_bkgd[0] != 0.f || opts->render_bkgd[1] != 0.f || opts->render_bkgd[2] != 0.f ? w.scalars->bkgd : nullptr;
}

inline int fill_blocks(int rblocks) { return rblocks > 2048 ? rblocks : 2048; }      // enough threads for the 50 MB gradient fill (16 bytes per thread and pass)

// What an entry point hands down unchanged, in BackwardCall's manner (the backward entry points have no grid and no rays, a presample no max_kept and no report words)
struct StepCall {
    const uint8_t *binaries; const uint32_t *bitgrid; const float *occs; int32_t res_x, res_y, res_z;
    const float *aabb_host, *rays_o, *rays_d; int32_t n_rays;
    const mnf_train_opts *opts;
    int64_t max_marched, max_kept;
    int64_t *counts_dev; int32_t *skip_dev;
    hipStream_t stream;
};

// The argument checks the entry points share, under the entry point's name: handle and options and the options' size, in front of an entry point's own checks ...
int check_args(const char *who, bool handles, const mnf_train_opts *opts) {
    MNF_REQUIRE(handles && opts, "%s: bad handle or options", who);
    MNF_REQUIRE(opts->struct_size == sizeof(mnf_train_opts), "%s: opts->struct_size is %u, this library's mnf_train_opts has %zu bytes (MNF_INIT)", who,
                opts->struct_size, sizeof(mnf_train_opts));
    return MNF_OK;
}
// ... and behind them: positive sizes (`option`: the option that has to be positive too), the carve, the workspace's size (check_workspace)
int open_step(const char *who, mnf_field_t f, const StepCall &c, float option, void *workspace, int64_t workspace_bytes, StepWs &w) {
    MNF_REQUIRE(c.n_rays > 0 && c.max_marched > 0 && c.max_kept > 0 && option > 0.f, "%s: bad sizes", who);
    w = carve_step(workspace, f, c.n_rays, scratch_cap(c.n_rays), c.max_marched, c.max_kept);
    return check_workspace(who, workspace, workspace_bytes, w.bytes);
}

// near planes, alpha threshold, march, offsets, longest ray, bound check (its counters and flag: `report`, `skip`), packing: what reads rays and grid but no parameter
int sample_stage(const StepCall &c, const SampleWs &w, float *losses, const StepFills &fills, int64_t *report, int32_t *skip) {
    const int64_t cells = (int64_t)c.res_x * c.res_y * c.res_z;
    const int rblocks = (c.n_rays + 255) / 256;
    const int32_t cap = scratch_cap(c.n_rays);
    hipLaunchKernelGGL(planes_kernel, dim3(losses ? fill_blocks(rblocks) : rblocks), dim3(256), 0, c.stream, c.n_rays, c.opts->near_plane, c.opts->far_plane,
                       c.opts->render_step_size, c.opts->stratified, (uint32_t)c.opts->seed, (uint32_t)(c.opts->seed >> 32), w.nearp, w.farp, losses, c.counts_dev, c.skip_dev, fills);
    const int n_levels = c.opts->n_levels > 1 ? c.opts->n_levels : 1;
    hipLaunchKernelGGL(mean_partial_kernel, dim3(128), dim3(256), 0, c.stream, c.occs, cells * n_levels, w.words->mean_part);          // occ_grid.py:192: the mean over every level
    hipLaunchKernelGGL(mean_final_kernel, dim3(1), dim3(64), 0, c.stream, (const double *)w.words->mean_part, 128, cells * n_levels, c.opts->alpha_thre,
                       &w.scalars->alpha_thre);
    if (const int rc = mnf_sample_rays_levels(c.rays_o, c.rays_d, c.n_rays, c.binaries, n_levels, c.res_x, c.res_y, c.res_z, c.aabb_host, w.nearp, w.farp, c.opts->render_step_size,
                                    c.opts->cone_angle, cap, w.scratch_ts, w.scratch_te, w.counts, c.bitgrid, (mnf_stream_t)c.stream))
        return rc;
    if (const int rc = mnf_exclusive_scan_i64(w.counts, c.n_rays, w.starts, &w.words->marched, w.scan, mnf_scan_workspace_bytes(c.n_rays), (mnf_stream_t)c.stream)) return rc;
    hipLaunchKernelGGL(max_kernel, dim3(1), dim3(1024), 0, c.stream, w.counts, (int64_t)c.n_rays, &w.words->longest);
    // a ray longer than its scratch row would have been truncated (the rows hold `cap` samples; the reference configurations stay far
    // below) and more marched samples than `max_marched` would not fit the packed arrays: both end the step here, on the device
    hipLaunchKernelGGL(guard_marched_kernel, dim3(rblocks), dim3(256), 0, c.stream, c.n_rays, w.counts, w.starts, (const int64_t *)&w.words->marched, c.max_marched,
                       (int64_t)cap, eff_counts(w), report, skip);
    if (const int rc = launch_status("sample_stage")) return rc;
    return mnf_compact_samples(w.scratch_ts, w.scratch_te, cap, w.starts, w.counts, c.n_rays, w.ts, w.te, w.ray, (mnf_stream_t)c.stream);
}

}  // namespace

// For the pose refiner (localize.hip), which decides per VIEW whether anything was rendered: where a step's workspace keeps every ray's surviving-sample
// count (visibility_kernel's; zeroed by the guards).  Intact from the forward to behind its backward.
const int64_t *train_step_kept_counts(void *workspace, mnf_field_t f, int32_t n_rays, int64_t max_marched, int64_t max_kept) {
    return carve_step(workspace, f, n_rays, scratch_cap(n_rays), max_marched, max_kept).kept_cnts;
}
}  // namespace mnf

using namespace mnf;

extern "C" int mnf_visible_samples(const int64_t *chunk_starts, const int64_t *chunk_cnts, int32_t n_rays, const float *t_starts, const float *t_ends,
                                   const float *sigmas, float early_stop_eps, const float *alpha_thre_dev, int64_t *kept_cnts, const int64_t *kept_starts,
                                   float *o_t_starts, float *o_t_ends, int64_t *o_ray_indices, mnf_stream_t stream) {
    if (n_rays <= 0) return MNF_OK;
    MNF_REQUIRE(chunk_starts && chunk_cnts && t_starts && t_ends && sigmas && alpha_thre_dev, "visible_samples: null pointer");
    const int vgrid = n_rays < 65535 ? n_rays : 65535;
    if (!o_t_starts) {
        MNF_REQUIRE(kept_cnts, "visible_samples: the count pass needs kept_cnts");
        hipLaunchKernelGGL(visibility_kernel<false>, dim3(vgrid), dim3(64), 0, as_stream(stream), n_rays, chunk_starts, chunk_cnts, t_starts, t_ends, sigmas, early_stop_eps,
                           alpha_thre_dev, kept_cnts, (const int64_t *)nullptr, (float *)nullptr, (float *)nullptr, (int64_t *)nullptr, (int64_t *)nullptr);
    } else {
        MNF_REQUIRE(kept_starts && o_t_ends && o_ray_indices, "visible_samples: the write pass needs kept_starts and the three outputs");
        hipLaunchKernelGGL(visibility_kernel<true>, dim3(vgrid), dim3(64), 0, as_stream(stream), n_rays, chunk_starts, chunk_cnts, t_starts, t_ends, sigmas, early_stop_eps,
                           alpha_thre_dev, (int64_t *)nullptr, kept_starts, o_t_starts, o_t_ends, o_ray_indices, (int64_t *)nullptr);
    }
    return launch_status("visibility_kernel");
}

extern "C" int64_t mnf_train_step_workspace_bytes(mnf_field_t f, int32_t n_rays, int64_t max_marched, int64_t max_kept) {
    if (!f || n_rays <= 0 || max_marched <= 0 || max_kept <= 0) return -1;
    return carve_step(nullptr, f, n_rays, scratch_cap(n_rays), max_marched, max_kept).bytes;
}

extern "C" int mnf_presample_create(mnf_presample_t *out) {
    MNF_REQUIRE(out, "presample_create: null pointer");
    mnf_presample_s *p = new mnf_presample_s();
    if (hipEventCreateWithFlags(&p->ev_ready, hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&p->ev_done, hipEventDisableTiming) != hipSuccess) {
        if (p->ev_ready) (void)hipEventDestroy(p->ev_ready);
        delete p;
        set_error("presample_create: hipEventCreate failed");
        return MNF_ERR_HIP;
    }
    *out = p;
    return MNF_OK;
}

extern "C" void mnf_presample_destroy(mnf_presample_t p) {
    if (!p) return;
    (void)hipEventDestroy(p->ev_ready);
    (void)hipEventDestroy(p->ev_done);
    delete p;
}

extern "C" int64_t mnf_train_presample_workspace_bytes(int32_t n_rays, int64_t max_marched) {
    if (n_rays <= 0 || max_marched <= 0) return -1;
    return carve_sample(nullptr, n_rays, scratch_cap(n_rays), max_marched).bytes;
}

extern "C" int mnf_presample_wait(mnf_presample_t p, mnf_stream_t stream) {
    MNF_REQUIRE(p, "presample_wait: null handle");
    if (p->launched) MNF_HIP(hipStreamWaitEvent(as_stream(stream), p->ev_done, 0));
    return MNF_OK;
}

extern "C" int mnf_train_presample(mnf_presample_t p, const uint8_t *binaries, const uint32_t *bitgrid, const float *occs, int32_t res_x, int32_t res_y,
                                   int32_t res_z, const float *aabb_host, const float *rays_o, const float *rays_d, int32_t n_rays,
                                   const mnf_train_opts *opts, int64_t max_marched, void *workspace, int64_t workspace_bytes, mnf_stream_t stream) {
    MNF_REQUIRE(p && binaries && occs && aabb_host && rays_o && rays_d && opts && workspace, "train_presample: null pointer");
    if (const int rc = check_args("train_presample", true, opts)) return rc;
    MNF_REQUIRE(n_rays > 0 && max_marched > 0 && opts->render_step_size > 0.f, "train_presample: bad sizes");      // (a presample filters nothing: no max_kept)
    const int n_levels = opts->n_levels > 1 ? opts->n_levels : 1;
    MNF_REQUIRE(n_levels <= 4, "train_presample: at most 4 occupancy levels");
    const SampleWs w = carve_sample(workspace, n_rays, scratch_cap(n_rays), max_marched);
    if (const int rc = check_workspace("train_presample", workspace, workspace_bytes, w.bytes)) return rc;
    hipStream_t s = as_stream(stream), ss = shared_side_stream(2);
    if (!ss) return MNF_ERR_HIP;
    StepCall c = {};      // (its stream: the side stream the march runs on)
    c.binaries = binaries; c.bitgrid = bitgrid; c.occs = occs; c.res_x = res_x; c.res_y = res_y; c.res_z = res_z; c.aabb_host = aabb_host;
    c.rays_o = rays_o; c.rays_d = rays_d; c.n_rays = n_rays; c.opts = opts; c.max_marched = max_marched; c.stream = ss;
    p->valid = 0;
    // fork: the side stream continues from the caller's stream as it is NOW — in front of whatever the caller enqueues next (the step this march is to hide behind)
    MNF_HIP(hipEventRecord(p->ev_ready, s));
    MNF_HIP(hipStreamWaitEvent(ss, p->ev_ready, 0));
    const int rc = sample_stage(c, w, nullptr, StepFills{}, w.words->pre_report, nullptr);      // (the bound check's counters go to the handle's own words: the adopting step copies them)
    MNF_HIP(hipEventRecord(p->ev_done, ss));
    p->launched = 1;
    if (rc) return rc;
    p->ws = workspace; p->rays_o = rays_o; p->rays_d = rays_d; p->binaries = binaries; p->n_rays = n_rays; p->seed = opts->seed; p->stratified = opts->stratified;
    p->n_levels = n_levels; p->near_plane = opts->near_plane; p->far_plane = opts->far_plane; p->step = opts->render_step_size; p->cone = opts->cone_angle;
    p->alpha_thre = opts->alpha_thre; p->res[0] = res_x; p->res[1] = res_y; p->res[2] = res_z; p->max_marched = max_marched;
    p->valid = 1;
    return MNF_OK;
}

namespace mnf {
namespace {
// A step in front of its loss — planes and fills, alpha threshold, march, guards, compaction, ray-major density pre-pass leaving its feature rows, visibility filter,
// forward_train reading the rows, compositing forward — and behind it.  mnf_train_step is the two with loss_kernel in between; mnf_train_render_forward /
// _backward are the same two with the caller's own loss in between.  Whatever the second half reads of the first lies in `w` (its march's part: see kept_scan).
int step_forward(mnf_field_t f, const StepCall &c, StepWs &w, StepFills fills, float *losses) {
    const int C = f->cfg.num_semantic_classes;
    const int rblocks = (c.n_rays + 255) / 256;
    // (losses, counters, skip flag, the three gradient vectors, the pre-pass's density array and work counter: zeroed by planes_kernel)
    // ---- occupancy sampling (occ_grid.py:80-238): march, density pre-pass, visibility filter
    const int n_levels = c.opts->n_levels > 1 ? c.opts->n_levels : 1;
    MNF_REQUIRE(n_levels <= 4, "train_step: at most 4 occupancy levels");
    if (const mnf_presample_s *pre = c.opts->presampled) {
        // the march of THIS batch ran earlier, on a side stream beside the previous step (mnf_train_presample): adopt what it left, after its last kernel
        MNF_REQUIRE(pre->valid && pre->rays_o == c.rays_o && pre->rays_d == c.rays_d && pre->n_rays == c.n_rays && pre->binaries == c.binaries && pre->seed == c.opts->seed &&
                    pre->stratified == c.opts->stratified && pre->n_levels == n_levels && pre->near_plane == c.opts->near_plane && pre->far_plane == c.opts->far_plane &&
                    pre->step == c.opts->render_step_size && pre->cone == c.opts->cone_angle && pre->alpha_thre == c.opts->alpha_thre &&
                    pre->res[0] == c.res_x && pre->res[1] == c.res_y && pre->res[2] == c.res_z && pre->max_marched == c.max_marched,
                    "train_step: opts->presampled was made for other rays, options, sample bound or another grid");
        if (hipEventQuery(pre->ev_done) != hipSuccess) MNF_HIP(hipStreamWaitEvent(c.stream, pre->ev_done, 0));      // (a wait on another queue costs the stream ~18 us even when the event is long done)
        static_cast<SampleWs &>(w) = carve_sample(pre->ws, c.n_rays, scratch_cap(c.n_rays), c.max_marched);      // (the two small blocks included: every word of this step is the presample's)
        const_cast<mnf_presample_s *>(pre)->valid = 0;      // (the guards below may clear its counts: one use)
        fills.ray_counter = &w.words->ray_counter;
        fills.adopt = w.words->pre_report;
        hipLaunchKernelGGL(planes_kernel, dim3(fill_blocks(rblocks)), dim3(256), 0, c.stream, 0, 0.f, 0.f, 0.f, 0, 0u, 0u, (float *)nullptr, (float *)nullptr, losses, c.counts_dev,
                           c.skip_dev, fills);
    } else {      // (a presample has done all three)
        fills.ray_counter = &w.words->ray_counter;
        if (const int rc = sample_stage(c, w, losses, fills, c.counts_dev, c.skip_dev)) return rc;
    }
    int64_t *eff = eff_counts(w);
    bool use_rows = false;
    FieldIO pp = {};      // the density pre-pass over the marched samples
    pp.rays_o = c.rays_o; pp.rays_d = c.rays_d; pp.ray_idx64 = w.ray; pp.t_starts = w.ts; pp.t_ends = w.te; pp.n = c.max_marched; pp.density = w.sigma;
    static const bool prepass_flat = diag_env("MNF_PREPASS_FLAT") != nullptr;    // experiment: every marched sample, full lanes, no early termination
    if (prepass_flat) {
        pp.mode = 1; pp.n_dev64 = eff;
    } else {
        // mnf_field_density_rays without its two memsets (density array, work counter: planes_kernel's fills): ray-major, skips what lies behind T < eps / 2
        pp.mode = 3; pp.chunk_starts = w.starts; pp.chunk_cnts = w.counts; pp.n_rays = c.n_rays; pp.ray_counter = fills.ray_counter;
        pp.sdt_stop = c.opts->early_stop_eps > 0.0f ? -logf(c.opts->early_stop_eps) + 0.6931472f : INFINITY;
        static const bool no_rows = diag_env("MNF_NO_ROWS") != nullptr;      // A/B timing: both passes gather
        use_rows = w.rows != nullptr && !no_rows;
        pp.rows_out = use_rows ? w.rows : nullptr;       // (NULL where the rows are not built: the forward then gathers for itself)
    }
    if (const int rc = launch_field(f, pp, true, c.stream)) return rc;
    const int vgrid = c.n_rays < 65535 ? c.n_rays : 65535;
    hipLaunchKernelGGL(visibility_kernel<false>, dim3(vgrid), dim3(64), 0, c.stream, c.n_rays, w.starts, w.counts, w.ts, w.te, w.sigma, c.opts->early_stop_eps,
                       &w.scalars->alpha_thre, w.kept_cnts, (const int64_t *)nullptr, (float *)nullptr, (float *)nullptr, (int64_t *)nullptr, (int64_t *)nullptr);
    if (const int rc = mnf_exclusive_scan_i64(w.kept_cnts, c.n_rays, w.kept_starts, &w.words->kept, w.kept_scan, mnf_scan_workspace_bytes(c.n_rays), (mnf_stream_t)c.stream)) return rc;
    hipLaunchKernelGGL(guard_kept_kernel, dim3(rblocks), dim3(256), 0, c.stream, c.n_rays, w.kept_cnts, w.kept_starts, (const int64_t *)&w.words->marched, c.max_kept, eff,
                       c.counts_dev, c.skip_dev);
    hipLaunchKernelGGL(visibility_kernel<true>, dim3(vgrid), dim3(64), 0, c.stream, c.n_rays, w.starts, w.counts, w.ts, w.te, w.sigma, c.opts->early_stop_eps,
                       &w.scalars->alpha_thre, (int64_t *)nullptr, w.kept_starts, w.k_ts, w.k_te, w.k_ray, use_rows ? w.k_src : (int64_t *)nullptr);
    // ---- sem_rendering (utils.py:362-461): field with saved activations, compositing
    {
        FieldIO io = {};
        io.mode = 1; io.rays_o = c.rays_o; io.rays_d = c.rays_d; io.ray_idx64 = w.k_ray; io.t_starts = w.k_ts; io.t_ends = w.k_te;
        io.n = c.max_kept; io.n_dev64 = &eff[1];
        io.rgb = w.k_rgb; io.density = w.k_sigma; io.sem = w.k_sem; io.xn_out = w.k_pos;        // aabb-normalised: what the backward's scatter reads
        io.sem_stride = c.max_kept;                                                                // the step's own logit buffer is class-major: w.k_sem[class * max_kept + sample]
        if (use_rows) { io.rows_in = w.rows; io.rows_src = w.k_src; }                            // every survivor's features: the row the pre-pass left, not 128 gathers
        if (const int rc = forward_train(f, io, w.field_ws, w.field_ws_bytes, c.stream, c.opts->deterministic != 0)) return rc;
    }
    const float *bk = background(w, c.opts);
    if (bk && !c.opts->render_bkgd_dev)      // the by-value colour, into its three floats of the small scalar block
        hipLaunchKernelGGL(set3_kernel, dim3(1), dim3(1), 0, c.stream, w.scalars->bkgd, c.opts->render_bkgd[0], c.opts->render_bkgd[1], c.opts->render_bkgd[2]);
    return composite_train_forward_impl(w.kept_starts, w.kept_cnts, c.n_rays, w.k_ts, w.k_te, w.k_sigma, w.k_rgb, w.k_sem, c.max_kept, C, c.max_kept, bk, w.o_rgb, w.o_acc,
                                        w.o_dep, w.o_sem, w.k_w, w.k_tr, nullptr, (mnf_stream_t)c.stream);
}

// composite_train_backward (g_acc: the caller's opacity gradient, or NULL), the factored output gradient, the field's backward
int step_backward(mnf_field_t f, const StepCall &sc, const StepWs &w, const float *g_acc, float *g_base, float *g_head, float *g_sem) {
    const int C = f->cfg.num_semantic_classes;
    // the rgb / semantic output gradients of a sample are its weight times its ray's loss gradient: the split backward forms them itself from (k_w, k_ray, g_rgb, g_sem)
    // — 12 bytes per sample and cached per-ray vectors instead of 128 bytes written here and read there; the fused backward (mode 2) reads the per-sample arrays
    const bool factored = C > 0;
    int rc = composite_train_backward_impl(w.kept_starts, w.kept_cnts, sc.n_rays, w.k_ts, w.k_te, w.k_sigma, w.k_rgb, w.k_sem, sc.max_kept, C, sc.max_kept, background(w, sc.opts),
                                           w.k_w, w.k_tr, w.o_acc, w.o_dep, w.g_rgb, g_acc, w.g_dep, w.g_sem, w.k_dsig, factored ? nullptr : w.k_drgb,
                                           factored ? nullptr : w.k_dsem, (mnf_stream_t)sc.stream);
    if (rc) return rc;
    BackwardCall c = {};
    c.positions = w.k_pos; c.n = sc.max_kept; c.n_dev = &eff_counts(w)[1]; c.d_rgb = w.k_drgb; c.d_density = w.k_dsig; c.d_sem = w.k_dsem; c.rgb = w.k_rgb; c.density = w.k_sigma;
    c.workspace = w.field_ws; c.workspace_bytes = w.field_ws_bytes; c.loss_scale = sc.opts->loss_scale; c.g_base = g_base; c.g_head = g_head; c.g_sem = g_sem;
    c.positions_normalized = true; c.deterministic = sc.opts->deterministic != 0; c.stream = sc.stream;
    if (factored) c.factored = FactoredGrad{w.k_w, w.k_ray, w.g_rgb, w.g_sem};
    return backward(f, c);
}

// What the two backward entry points share behind their argument checks: the head (gradients_in_kernel) and step_backward
int render_backward(mnf_field_t f, const StepCall &c, const StepWs &w, const GradIn &i_rgb, const GradIn &i_acc, const GradIn &i_dep, const GradIn &i_sem, float *g_base,
                    float *g_head, float *g_sem_params) {
    const GradFills z = {g_base, g_head, g_sem_params, (int64_t)f->n_base, (int64_t)f->n_head, (int64_t)f->n_sem};
    hipLaunchKernelGGL(gradients_in_kernel, dim3(fill_blocks((c.n_rays + 255) / 256)), dim3(256), 0, c.stream, c.n_rays, f->cfg.num_semantic_classes, i_rgb, i_acc,
                       i_dep, i_sem, w.g_rgb, w.g_acc, w.g_dep, w.g_sem, z, c.counts_dev, c.skip_dev, eff_counts(w), &w.words->ticket);
    if (const int rc = launch_status("gradients_in_kernel")) return rc;
    return step_backward(f, c, w, w.g_acc, g_base, g_head, g_sem_params);
}
}  // namespace
}  // namespace mnf

extern "C" int mnf_train_step(mnf_field_t f, const uint8_t *binaries, const uint32_t *bitgrid, const float *occs, int32_t res_x, int32_t res_y,
                              int32_t res_z, const float *aabb_host, const float *rays_o, const float *rays_d, int32_t n_rays,
                              const float *target_rgb, const float *target_depth, const int64_t *target_sem, const mnf_train_opts *opts,
                              float *g_base, float *g_head, float *g_sem, float *losses, int64_t *counts_dev, int32_t *skip_dev, int64_t max_marched,
                              int64_t max_kept, void *workspace, int64_t workspace_bytes, mnf_stream_t stream) {
    if (const int rc = check_args("train_step", f && f->params_loaded && aabb_host && counts_dev && skip_dev, opts)) return rc;
    MNF_REQUIRE(binaries && occs && rays_o && rays_d && target_rgb && target_depth && target_sem && g_base && g_head && g_sem && losses && workspace,
                "train_step: null pointer");
    StepCall c = {};
    c.binaries = binaries; c.bitgrid = bitgrid; c.occs = occs; c.res_x = res_x; c.res_y = res_y; c.res_z = res_z; c.aabb_host = aabb_host; c.rays_o = rays_o; c.rays_d = rays_d;
    c.n_rays = n_rays; c.opts = opts; c.max_marched = max_marched; c.max_kept = max_kept; c.counts_dev = counts_dev; c.skip_dev = skip_dev; c.stream = as_stream(stream);
    StepWs w;
    if (const int rc = open_step("train_step", f, c, opts->render_step_size, workspace, workspace_bytes, w)) return rc;
    const StepFills fills = {g_base, g_head, g_sem, w.sigma, (int64_t)f->n_base, (int64_t)f->n_head, (int64_t)f->n_sem, max_marched, nullptr, nullptr};
    if (const int rc = step_forward(f, c, w, fills, losses)) return rc;
    // ---- loss (pipeline.py:506-511) and backward (pipeline.py:518)
    hipLaunchKernelGGL(loss_kernel, dim3((n_rays + 255) / 256), dim3(256), 0, c.stream, n_rays, f->cfg.num_semantic_classes, w.o_rgb, w.o_dep, w.o_sem, target_rgb,
                       target_depth, target_sem, w.g_rgb, w.g_dep, w.g_sem, losses, counts_dev + 3, skip_dev);
    if (const int rc = launch_status("loss_kernel")) return rc;
    return step_backward(f, c, w, nullptr, g_base, g_head, g_sem);
}

// The step cut at its loss (include/mi355nerf.h): step_forward now, step_backward later with the caller's gradients, from the same workspace
extern "C" int mnf_train_render_forward(mnf_field_t f, const uint8_t *binaries, const uint32_t *bitgrid, const float *occs, int32_t res_x, int32_t res_y,
                                        int32_t res_z, const float *aabb_host, const float *rays_o, const float *rays_d, int32_t n_rays,
                                        const mnf_train_opts *opts, float *rgb, float *acc, float *depth, float *sem, int64_t *counts_dev, int32_t *skip_dev,
                                        int64_t max_marched, int64_t max_kept, void *workspace, int64_t workspace_bytes, mnf_stream_t stream) {
    if (const int rc = check_args("train_render_forward", f && f->params_loaded && aabb_host && counts_dev && skip_dev, opts)) return rc;
    MNF_REQUIRE(!opts->presampled, "train_render_forward: opts->presampled must be NULL (a presampled march is adopted by mnf_train_step only)");
    MNF_REQUIRE(binaries && occs && rays_o && rays_d && rgb && acc && depth && workspace, "train_render_forward: null pointer");
    MNF_REQUIRE(sem || f->cfg.num_semantic_classes == 0, "train_render_forward: null pointer (sem may be NULL only for a field without semantic classes)");
    MNF_REQUIRE(opts->n_levels <= 4, "train_render_forward: at most 4 occupancy levels");
    StepCall c = {};
    c.binaries = binaries; c.bitgrid = bitgrid; c.occs = occs; c.res_x = res_x; c.res_y = res_y; c.res_z = res_z; c.aabb_host = aabb_host; c.rays_o = rays_o; c.rays_d = rays_d;
    c.n_rays = n_rays; c.opts = opts; c.max_marched = max_marched; c.max_kept = max_kept; c.counts_dev = counts_dev; c.skip_dev = skip_dev; c.stream = as_stream(stream);
    StepWs w;
    if (const int rc = open_step("train_render_forward", f, c, opts->render_step_size, workspace, workspace_bytes, w)) return rc;
    const StepFills fills = {nullptr, nullptr, nullptr, w.sigma, 0, 0, 0, max_marched, nullptr, nullptr};      // (no gradient vector is touched here)
    if (const int rc = step_forward(f, c, w, fills, w.scalars->render_losses)) return rc;
    // (a guard that fired has cleared every per-ray count: the compositing then wrote the background colour and zeros, never what the workspace held before)
    const int C = f->cfg.num_semantic_classes;
    const int64_t widest = (int64_t)n_rays * (C > 3 ? C : 3);
    hipLaunchKernelGGL(outputs_kernel, dim3((unsigned)((widest + 255) / 256)), dim3(256), 0, c.stream, (int64_t)n_rays, C, w.o_rgb, w.o_acc, w.o_dep, w.o_sem,
                       rgb, acc, depth, sem, skip_dev, &w.words->ticket);
    return launch_status("outputs_kernel");
}

extern "C" int mnf_train_render_backward(mnf_field_t f, int32_t n_rays, const mnf_train_opts *opts, const float *g_rgb, int64_t g_rgb_row_stride,
                                         int64_t g_rgb_col_stride, const float *g_acc, int64_t g_acc_row_stride, const float *g_depth, int64_t g_depth_row_stride,
                                         const float *g_sem, int64_t g_sem_row_stride, int64_t g_sem_col_stride, float *g_base, float *g_head, float *g_sem_params,
                                         int64_t *counts_dev, int32_t *skip_dev, int64_t max_marched, int64_t max_kept, void *workspace, int64_t workspace_bytes,
                                         mnf_stream_t stream) {
    if (const int rc = check_args("train_render_backward", f && f->params_loaded && counts_dev && skip_dev, opts)) return rc;
    MNF_REQUIRE(!opts->presampled, "train_render_backward: opts->presampled must be NULL");
    MNF_REQUIRE(g_base && g_head && g_sem_params && workspace, "train_render_backward: null pointer");
    StepCall c = {};
    c.n_rays = n_rays; c.opts = opts; c.max_marched = max_marched; c.max_kept = max_kept; c.counts_dev = counts_dev; c.skip_dev = skip_dev; c.stream = as_stream(stream);
    StepWs w;
    if (const int rc = open_step("train_render_backward", f, c, 1.f, workspace, workspace_bytes, w)) return rc;      // (no option of its own has to be positive)
    return render_backward(f, c, w, GradIn{g_rgb, g_rgb_row_stride, g_rgb_col_stride}, GradIn{g_acc, g_acc_row_stride, 0}, GradIn{g_depth, g_depth_row_stride, 0},
                           GradIn{g_sem, g_sem_row_stride, g_sem_col_stride}, g_base, g_head, g_sem_params);
}

// mnf_train_render_backward, then the ray gradients from what it left in the workspace (inputgrad.hip).  The three parameter pointers all NULL: the parameters are
// frozen — the head fills nothing and the field's backward stops behind dgrad (train.hip backward_impl).
extern "C" int mnf_train_render_backward_rays(mnf_field_t f, int32_t n_rays, const mnf_train_opts *opts, const float *rays_d, const float *g_rgb,
                                              int64_t g_rgb_row_stride, int64_t g_rgb_col_stride, const float *g_acc, int64_t g_acc_row_stride, const float *g_depth,
                                              int64_t g_depth_row_stride, const float *g_sem, int64_t g_sem_row_stride, int64_t g_sem_col_stride, float *g_base,
                                              float *g_head, float *g_sem_params, float *g_rays_o, float *g_rays_d, int64_t *counts_dev, int32_t *skip_dev,
                                              int64_t max_marched, int64_t max_kept, void *workspace, int64_t workspace_bytes, mnf_stream_t stream) {
    if (const int rc = check_args("train_render_backward_rays", f && f->params_loaded && counts_dev && skip_dev, opts)) return rc;
    MNF_REQUIRE(!opts->presampled, "train_render_backward_rays: opts->presampled must be NULL");
    MNF_REQUIRE(g_rays_o || g_rays_d, "train_render_backward_rays: no ray gradient asked for (mnf_train_render_backward is the call without)");
    MNF_REQUIRE(!g_rays_d || rays_d, "train_render_backward_rays: g_rays_d needs rays_d, the directions the forward was given");
    const bool frozen = !g_base && !g_head && !g_sem_params;
    MNF_REQUIRE(frozen || (g_base && g_head && g_sem_params), "train_render_backward_rays: the three parameter gradients are given together, or all NULL (frozen)");
    StepCall c = {};
    c.n_rays = n_rays; c.opts = opts; c.max_marched = max_marched; c.max_kept = max_kept; c.counts_dev = counts_dev; c.skip_dev = skip_dev; c.stream = as_stream(stream);
    StepWs w;
    if (const int rc = open_step("train_render_backward_rays", f, c, opts->loss_scale, workspace, workspace_bytes, w)) return rc;
    if (const int rc = render_backward(f, c, w, GradIn{g_rgb, g_rgb_row_stride, g_rgb_col_stride}, GradIn{g_acc, g_acc_row_stride, 0}, GradIn{g_depth, g_depth_row_stride, 0},
                                       GradIn{g_sem, g_sem_row_stride, g_sem_col_stride}, g_base, g_head, g_sem_params))
        return rc;
    RayGradIO io = {};
    io.xn = w.k_pos; io.t_starts = w.k_ts; io.t_ends = w.k_te; io.kept_starts = w.kept_starts; io.kept_cnts = w.kept_cnts;
    io.n_dev = &eff_counts(w)[1]; io.skip = skip_dev; io.rays_d = rays_d; io.n_rays = n_rays; io.n = max_kept; io.loss_scale = opts->loss_scale;
    io.g_o = g_rays_o; io.g_d = g_rays_d;
    return train_render_ray_grad(f, w.field_ws, io, c.stream);
}
