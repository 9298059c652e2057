// Batched pose refinement against the frozen map (include/mi355nerf.h: "pose refinement"): B views, each with its own 6-vector correction
// xi[b] = (rotvec, trans) of its initial pose c2w0[b], a whole run of iterations as ONE C call and no host synchronisation inside the run.
//
//   mnf_pose_rays     pose_rays_kernel: pixel draw (or the caller's pixels), the rays of raygen_kernel (march.hip) under the current correction — what
//                     render.transform_rays does to a view's rays — and the targets of gather_pixels_kernel, for B views x n rays in one launch
//   mnf_pose_loss     pose_loss_kernel: the per-view three-term loss of loss_kernel (trainstep.hip; pipeline.py:506-511) and its plane gradients,
//                     one workgroup per view, every mean over the view's own n rays
//   mnf_pose_update   pose_update_kernel: the view's ray gradients summed to the 6-vector gradient in float64 in a fixed order, one Adam step on it;
//                     one workgroup per view
//   mnf_pose_refine   per iteration: pose_rays, mnf_train_render_forward's launches, pose_loss, mnf_train_render_backward_rays' launches with the
//                     parameters frozen, pose_update.  All B n rays go through one forward and one backward.
//
// Built with -ffp-contract=off: a ray is a chain of separately rounded fp32 operations (tests/localize_ref.py restates them).
#include <cmath>
#include <cstddef>
#include <cstring>

#include "field.h"
#include "philox_dev.h"
#include "pixel_dev.h"
#include "reduce_dev.h"
#include "workspace.h"

namespace mnf {
// trainstep.hip: where a step's workspace keeps the surviving-sample count of every ray (zeroed when a guard fired)
const int64_t *train_step_kept_counts(void *workspace, mnf_field_t f, int32_t n_rays, int64_t max_marched, int64_t max_kept);

namespace {

constexpr int kLossThreads = 1024, kUpdateThreads = 256;
constexpr uint32_t kPixelTag = 0x706F7365u;      // the draw's own Philox tag ("pose")

// Rodrigues in float64, transform_rays' branches: R = I + a K + b K^2, a = sin t / t, b = (1 - cos t) / t^2, their Taylor series below t^2 = 1e-6
__device__ __forceinline__ void rodrigues(const double *k, double *R) {
    const double t2 = (k[0] * k[0] + k[1] * k[1]) + k[2] * k[2];
    double a, b;
    if (t2 < 1e-6) {
        a = (1.0 - t2 / 6.0) + t2 * t2 / 120.0;
        b = (0.5 - t2 / 24.0) + t2 * t2 / 720.0;
    } else {
        const double t = sqrt(t2);
        a = sin(t) / t;
        b = (1.0 - cos(t)) / t2;
    }
    const double x = k[0], y = k[1], z = k[2];
    // K^2 = k k^T - t^2 I
    R[0] = 1.0 + b * (x * x - t2); R[1] = -a * z + b * (x * y);    R[2] = a * y + b * (x * z);
    R[3] = a * z + b * (x * y);    R[4] = 1.0 + b * (y * y - t2); R[5] = -a * x + b * (y * z);
    R[6] = -a * y + b * (x * z);   R[7] = a * x + b * (y * z);    R[8] = 1.0 + b * (z * z - t2);
}

struct PoseRaysArgs {
    const uint8_t *images; const void *depths; const void *sems; int32_t depth_f16, sem_u8;
    int64_t n_images; const int64_t *image_ids;
    const float *c2w0; float focal; int32_t W, H;
    const int64_t *pix_idx; const double *xi;
    int32_t B, n; uint32_t iteration, s0, s1;
    float *rays_o, *rays_d; int64_t *pix_out; float *rot_out;
    float *t_rgb, *t_dep; int64_t *t_lab;
};

__global__ void __launch_bounds__(256) pose_rays_kernel(const PoseRaysArgs a) {
    const int64_t total = (int64_t)a.B * a.n, pixels = (int64_t)a.W * a.H;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)blockDim.x * gridDim.x) {
        const int32_t b = (int32_t)(i / a.n), r = (int32_t)(i - (int64_t)b * a.n);
        int64_t pix;
        if (a.pix_idx) {
            pix = a.pix_idx[i];
            pix = pix < 0 ? 0 : (pix >= pixels ? pixels - 1 : pix);      // (the caller's ids are checked on the host; no read leaves the image whatever they are)
        } else {
            const U4 rnd = philox4x32_10({(uint32_t)r, (uint32_t)b, a.iteration, kPixelTag}, a.s0, a.s1);
            const int64_t x = (int64_t)(((uint64_t)rnd.x * (uint64_t)a.W) >> 32), y = (int64_t)(((uint64_t)rnd.y * (uint64_t)a.H) >> 32);
            pix = y * a.W + x;
        }
        a.pix_out[i] = pix;
        // ---- the pixel's ray from c2w0[b] (pixel_dev.h: raygen_kernel's)
        const float *m = a.c2w0 + (int64_t)b * 12;
        float cam0, cam1, d[3];
        pixel_ray(pix % a.W, pix / a.W, a.W, a.H, a.focal, m, cam0, cam1, d);
        normalize_ray(d);
        const float d0 = d[0], d1 = d[1], d2 = d[2];
        // ---- the correction: R in float64 from the float64 xi, rounded once; d' = R d; o' = c + trans (the rotation about the common origin drops out)
        const double *k = a.xi + (int64_t)b * 6;
        double Rd[9];
        rodrigues(k, Rd);
        float R[9];
#pragma unroll
        for (int j = 0; j < 9; ++j) R[j] = (float)Rd[j];
        a.rays_d[3 * i] = (R[0] * d0 + R[1] * d1) + R[2] * d2;
        a.rays_d[3 * i + 1] = (R[3] * d0 + R[4] * d1) + R[5] * d2;
        a.rays_d[3 * i + 2] = (R[6] * d0 + R[7] * d1) + R[8] * d2;
        a.rays_o[3 * i] = (float)((double)m[3] + k[3]);
        a.rays_o[3 * i + 1] = (float)((double)m[7] + k[4]);
        a.rays_o[3 * i + 2] = (float)((double)m[11] + k[5]);
        if (r == 0 && a.rot_out) {
#pragma unroll
            for (int j = 0; j < 9; ++j) a.rot_out[(int64_t)b * 9 + j] = R[j];
        }
        // ---- the pixel's targets (pixel_dev.h: gather_pixels_kernel's), image image_ids[b]
        int64_t img = a.image_ids[b];
        img = img < 0 ? 0 : (img >= a.n_images ? a.n_images - 1 : img);
        const int64_t p = img * pixels + pix;
#pragma unroll
        for (int c = 0; c < 3; ++c) a.t_rgb[3 * i + c] = unit_u8(a.images[3 * p + c]);
        a.t_dep[i] = load_depth(a.depths, a.depth_f16, p);
        a.t_lab[i] = load_label(a.sems, a.sem_u8, p);
    }
}

// One workgroup per view.  Pass 1: any label of the view outside [0, C)?  Pass 2: loss terms and plane gradients of its n rays (pixel_dev.h's two halves; zero
// gradients for a flagged view), the terms summed in float64 (block_sum, reduce_dev.h).
__global__ void __launch_bounds__(kLossThreads) pose_loss_kernel(int32_t n, int32_t C, const float *__restrict__ rgb, const float *__restrict__ depth,
                                                                 const float *__restrict__ sem, const float *__restrict__ t_rgb, const float *__restrict__ t_dep,
                                                                 const int64_t *__restrict__ t_lab, float w_rgb, float w_dep, float w_sem,
                                                                 float *__restrict__ g_rgb, float *__restrict__ g_dep, float *__restrict__ g_sem,
                                                                 double *__restrict__ loss, int32_t *__restrict__ view_status, int64_t *status_word) {
    __shared__ double s_wave[kLossThreads / 64];
    const int32_t b = blockIdx.x;
    const int64_t base = (int64_t)b * n;
    int bad = 0;
    if (C > 0)
        for (int32_t r = threadIdx.x; r < n; r += kLossThreads) { const int64_t lab = t_lab[base + r]; bad |= (lab < 0 || lab >= C) ? 1 : 0; }
    bad = __syncthreads_or(bad);
    const float inv_n = 1.0f / (float)n;
    double l_rgb = 0.0, l_dep = 0.0, l_sem = 0.0;
    for (int32_t r = threadIdx.x; r < n; r += kLossThreads) {
        const int64_t i = base + r;
        l_dep += (double)ray_loss_planes(i, rgb, depth, t_rgb, t_dep, w_rgb / 3.0f, w_dep, inv_n, bad, g_rgb, g_dep, l_rgb);
        if (C > 0) l_sem += (double)ray_loss_sem(i, C, sem, t_lab, w_sem, inv_n, bad, g_sem, [] {});      // (the first pass has flagged a bad label)
    }
    const double s_rgb = block_sum<kLossThreads / 64>(l_rgb, s_wave), s_dep = block_sum<kLossThreads / 64>(l_dep, s_wave),
                 s_sem = block_sum<kLossThreads / 64>(l_sem, s_wave);
    if (threadIdx.x == 0) {
        loss[b] = ((double)w_rgb * (s_rgb / (3.0 * (double)n)) + (double)w_dep * (s_dep / (double)n)) + (double)w_sem * (s_sem / (double)n);
        view_status[b] = bad ? 8 : 0;
        if (bad && status_word) atomicOr(reinterpret_cast<unsigned long long *>(status_word), 8ull);
    }
}

struct PoseUpdateArgs {
    int32_t n; const float *g_o, *g_d, *rays_d; const int64_t *kept_cnts; const int32_t *view_status, *skip;
    double *xi, *m, *v; int32_t *stalled; double *grad_out;
    int64_t iteration;      // 0-based, counted over the whole refinement: the view's Adam step is iteration + 1 - stalled[b]
    double lr_rot, lr_trans, beta1, beta2, eps;
};

// One workgroup per view: S_o = sum g_o, S_w = sum d' x g_d over the view's rays in float64 (block_sum's fixed order: no atomics), then on one lane
// dL/dtrans = S_o, dL/drotvec = J_l(rotvec)^T S_w (J_l = I + b K + c K^2, so J_l^T v = v - b k x v + c k x (k x v)) and the Adam step.
__global__ void __launch_bounds__(kUpdateThreads) pose_update_kernel(const PoseUpdateArgs a) {
    __shared__ double s_wave[kUpdateThreads / 64];
    const int32_t b = blockIdx.x;
    const int64_t base = (int64_t)b * a.n;
    double s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    int kept = 0;
    for (int32_t r = threadIdx.x; r < a.n; r += kUpdateThreads) {
        const int64_t i = base + r;
        kept |= (!a.kept_cnts || a.kept_cnts[i] > 0) ? 1 : 0;
        const double go0 = a.g_o[3 * i], go1 = a.g_o[3 * i + 1], go2 = a.g_o[3 * i + 2];
        const double gd0 = a.g_d[3 * i], gd1 = a.g_d[3 * i + 1], gd2 = a.g_d[3 * i + 2];
        const double d0 = a.rays_d[3 * i], d1 = a.rays_d[3 * i + 1], d2 = a.rays_d[3 * i + 2];
        s[0] += go0; s[1] += go1; s[2] += go2;
        s[3] += d1 * gd2 - d2 * gd1; s[4] += d2 * gd0 - d0 * gd2; s[5] += d0 * gd1 - d1 * gd0;
    }
    kept = __syncthreads_or(kept);
#pragma unroll
    for (int j = 0; j < 6; ++j) s[j] = block_sum<kUpdateThreads / 64>(s[j], s_wave);
    if (threadIdx.x != 0) return;
    const double *k = a.xi + (int64_t)b * 6;
    const double t2 = (k[0] * k[0] + k[1] * k[1]) + k[2] * k[2];
    double cb, cc;
    if (t2 < 1e-6) {
        cb = (0.5 - t2 / 24.0) + t2 * t2 / 720.0;
        cc = (1.0 / 6.0 - t2 / 120.0) + t2 * t2 / 5040.0;
    } else {
        const double t = sqrt(t2);
        cb = (1.0 - cos(t)) / t2;
        cc = (t - sin(t)) / (t2 * t);
    }
    const double kx[3] = {k[1] * s[5] - k[2] * s[4], k[2] * s[3] - k[0] * s[5], k[0] * s[4] - k[1] * s[3]};              // k x S_w
    const double kkx[3] = {k[1] * kx[2] - k[2] * kx[1], k[2] * kx[0] - k[0] * kx[2], k[0] * kx[1] - k[1] * kx[0]};        // k x (k x S_w)
    double g[6];
#pragma unroll
    for (int j = 0; j < 3; ++j) { g[j] = (s[3 + j] - cb * kx[j]) + cc * kkx[j]; g[3 + j] = s[j]; }
    bool finite = true;
#pragma unroll
    for (int j = 0; j < 6; ++j) finite = finite && finite_d(g[j]);
    if (a.grad_out)
        for (int j = 0; j < 6; ++j) a.grad_out[(int64_t)b * 6 + j] = g[j];
    const bool stall = !kept || !finite || (a.view_status && a.view_status[b] != 0) || (a.skip && *a.skip > 0);
    if (stall) { a.stalled[b] += 1; return; }
    const double step = (double)(a.iteration + 1 - (int64_t)a.stalled[b]);
    const double bc1 = 1.0 - pow(a.beta1, step), bc2s = sqrt(1.0 - pow(a.beta2, step));
    double *x = a.xi + (int64_t)b * 6, *m = a.m + (int64_t)b * 6, *v = a.v + (int64_t)b * 6;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        const double lr = j < 3 ? a.lr_rot : a.lr_trans;
        m[j] = a.beta1 * m[j] + (1.0 - a.beta1) * g[j];
        v[j] = a.beta2 * v[j] + (1.0 - a.beta2) * (g[j] * g[j]);
        const double denom = sqrt(v[j]) / bc2s + a.eps;
        x[j] = x[j] - (lr / bc1) * (m[j] / denom);
    }
}

// ------------------------------------------------------------------ host side
int check_pose_opts(const char *who, const mnf_pose_opts *p) {
    MNF_REQUIRE(p, "%s: pose options are null", who);
    MNF_REQUIRE(p->struct_size == sizeof(mnf_pose_opts), "%s: pose->struct_size is %u, this library's mnf_pose_opts has %zu bytes (MNF_INIT)", who, p->struct_size,
                sizeof(mnf_pose_opts));
    MNF_REQUIRE(p->lr_rot >= 0.0 && p->lr_trans >= 0.0 && p->lr_rot <= 1.79e308 && p->lr_trans <= 1.79e308, "%s: learning rates must be finite and not negative", who);
    MNF_REQUIRE(p->beta1 >= 0.0 && p->beta1 < 1.0 && p->beta2 >= 0.0 && p->beta2 < 1.0 && p->eps > 0.0 && p->eps <= 1.79e308, "%s: need 0 <= beta < 1 and eps > 0", who);
    MNF_REQUIRE(p->w_rgb - p->w_rgb == 0.f && p->w_dep - p->w_dep == 0.f && p->w_sem - p->w_sem == 0.f, "%s: a loss weight is not finite", who);
    return MNF_OK;
}

int check_rays_args(const char *who, const uint8_t *images, const void *depths, const void *semantics, int64_t n_images, const int64_t *image_ids, const float *c2w0,
                    float focal, int32_t W, int32_t H, const double *xi, int32_t B, int32_t n) {
    MNF_REQUIRE(B > 0 && n > 0 && (int64_t)B * n <= 0x7fffffff, "%s: need n_views > 0, rays_per_view > 0 and at most 2^31 - 1 rays (got %d x %d)", who, B, n);
    MNF_REQUIRE(W > 0 && H > 0 && W <= 32768 && H <= 32768 && focal > 0.f && focal <= 3.4e38f, "%s: bad image size or focal (%d x %d, %g)", who, W, H, (double)focal);
    MNF_REQUIRE(n_images > 0, "%s: n_images must be positive", who);
    MNF_REQUIRE(images && depths && semantics && image_ids && c2w0 && xi, "%s: a null input pointer", who);
    MNF_REQUIRE(aligned8(image_ids) && aligned8(xi) && aligned4(c2w0), "%s: image_ids and xi must be 8-byte aligned, c2w0 4-byte", who);
    return MNF_OK;
}

// mnf_pose_refine's own part of the workspace, in front of the train step's
struct PoseWs {
    float *rays_o, *rays_d, *t_rgb, *t_dep, *rgb, *acc, *depth, *sem, *g_rgb, *g_dep, *g_sem, *g_o, *g_d, *rot;
    int64_t *pix, *t_lab;
    double *grad;
    int32_t *view_status, *skip;
    void *step_ws; int64_t step_bytes;
    size_t off[12];      // MNF_POSE_WS_*
    int64_t bytes;
};

PoseWs carve_pose(void *base, mnf_field_t f, int64_t B, int64_t n, int64_t max_marched, int64_t max_kept) {
    PoseWs w;
    Carver c(base);
    const size_t R = (size_t)(B * n), C = (size_t)f->cfg.num_semantic_classes;
    auto mark = [&](int k) { w.off[k] = c.off; };
    mark(0); w.rays_o = c.take<float>(R * 3); mark(1); w.rays_d = c.take<float>(R * 3); mark(2); w.pix = c.take<int64_t>(R);
    w.t_rgb = c.take<float>(R * 3); w.t_dep = c.take<float>(R); w.t_lab = c.take<int64_t>(R);
    mark(3); w.rgb = c.take<float>(R * 3); mark(4); w.acc = c.take<float>(R); mark(5); w.depth = c.take<float>(R); mark(6); w.sem = c.take<float>(R * (C ? C : 1));
    w.g_rgb = c.take<float>(R * 3); w.g_dep = c.take<float>(R); w.g_sem = c.take<float>(R * (C ? C : 1));
    mark(7); w.g_o = c.take<float>(R * 3); mark(8); w.g_d = c.take<float>(R * 3);
    mark(9); w.grad = c.take<double>((size_t)B * 6); mark(10); w.rot = c.take<float>((size_t)B * 9);
    w.view_status = c.take<int32_t>((size_t)B); w.skip = c.take<int32_t>(1);
    w.step_bytes = mnf_train_step_workspace_bytes(f, (int32_t)R, max_marched, max_kept);
    const size_t step_off = c.off;
    w.step_ws = c.take((size_t)(w.step_bytes > 0 ? w.step_bytes : 0));
    // (the step's kept counts: their place in its layout, found on a base nothing dereferences)
    char *const probe = reinterpret_cast<char *>(uintptr_t(1) << 20);
    w.off[11] = step_off + (size_t)(reinterpret_cast<const char *>(train_step_kept_counts(probe, f, (int32_t)R, max_marched, max_kept)) - probe);
    w.bytes = c.bytes();
    return w;
}

bool refine_sizes_ok(mnf_field_t f, int32_t B, int32_t n, int64_t max_marched, int64_t max_kept) {
    return f && B > 0 && n > 0 && (int64_t)B * n <= 0x7fffffff && max_marched > 0 && max_kept > 0;
}

int launch_pose_rays(const PoseRaysArgs &a, hipStream_t s) {
    ProfScope prof("pose_rays", s);
    hipLaunchKernelGGL(pose_rays_kernel, dim3(blocks_for((int64_t)a.B * a.n)), dim3(256), 0, s, a);
    return launch_status("pose_rays_kernel");
}

int launch_pose_loss(int32_t B, int32_t n, int32_t C, const float *rgb, const float *depth, const float *sem, const float *t_rgb, const float *t_dep, const int64_t *t_lab,
                     const mnf_pose_opts *p, float *g_rgb, float *g_dep, float *g_sem, double *loss, int32_t *view_status, int64_t *status_word, hipStream_t s) {
    ProfScope prof("pose_loss", s);
    hipLaunchKernelGGL(pose_loss_kernel, dim3((unsigned)B), dim3(kLossThreads), 0, s, n, C, rgb, depth, sem, t_rgb, t_dep, t_lab, p->w_rgb, p->w_dep, p->w_sem, g_rgb, g_dep,
                       g_sem, loss, view_status, status_word);
    return launch_status("pose_loss_kernel");
}

int launch_pose_update(int32_t B, const PoseUpdateArgs &a, hipStream_t s) {
    ProfScope prof("pose_update", s);
    hipLaunchKernelGGL(pose_update_kernel, dim3((unsigned)B), dim3(kUpdateThreads), 0, s, a);
    return launch_status("pose_update_kernel");
}

}  // namespace
}  // namespace mnf

using namespace mnf;

extern "C" int mnf_pose_rays(const uint8_t *images, const void *depths, int32_t depth_is_f16, const void *semantics, int32_t sem_is_u8, int64_t n_images,
                             const int64_t *image_ids, const float *c2w0, float focal, int32_t width, int32_t height, const int64_t *pix_idx, const double *xi,
                             int32_t n_views, int32_t rays_per_view, int64_t iteration, uint64_t seed, float *rays_o, float *rays_d, int64_t *pix_out, float *rot_out,
                             float *target_rgb, float *target_depth, int64_t *target_label, mnf_stream_t stream) {
    if (const int rc = check_rays_args("pose_rays", images, depths, semantics, n_images, image_ids, c2w0, focal, width, height, xi, n_views, rays_per_view)) return rc;
    MNF_REQUIRE(iteration >= 0 && iteration <= 0xffffffffll, "pose_rays: the iteration must fit 32 bits (got %lld)", (long long)iteration);
    MNF_REQUIRE(rays_o && rays_d && pix_out && target_rgb && target_depth && target_label, "pose_rays: a null output pointer");
    MNF_REQUIRE(aligned8(pix_out) && aligned8(target_label) && (!pix_idx || aligned8(pix_idx)), "pose_rays: pixel ids and labels must be 8-byte aligned");
    const PoseRaysArgs a = {images, depths, semantics, depth_is_f16, sem_is_u8, n_images, image_ids, c2w0, focal, width, height, pix_idx, xi, n_views, rays_per_view,
                            (uint32_t)iteration, (uint32_t)seed, (uint32_t)(seed >> 32), rays_o, rays_d, pix_out, rot_out, target_rgb, target_depth, target_label};
    return launch_pose_rays(a, as_stream(stream));
}

extern "C" int mnf_pose_loss(const float *rgb, const float *depth, const float *sem, const float *target_rgb, const float *target_depth, const int64_t *target_label,
                             int32_t n_views, int32_t rays_per_view, int32_t n_classes, const mnf_pose_opts *pose, double *loss, float *g_rgb, float *g_depth, float *g_sem,
                             int32_t *view_status, int64_t *status_word, mnf_stream_t stream) {
    if (const int rc = check_pose_opts("pose_loss", pose)) return rc;
    MNF_REQUIRE(n_views > 0 && rays_per_view > 0 && (int64_t)n_views * rays_per_view <= 0x7fffffff && n_classes >= 0, "pose_loss: bad sizes (%d views x %d rays, %d classes)",
                n_views, rays_per_view, n_classes);
    MNF_REQUIRE(rgb && depth && target_rgb && target_depth && loss && g_rgb && g_depth && view_status, "pose_loss: a null pointer");
    MNF_REQUIRE(n_classes == 0 || (sem && target_label && g_sem), "pose_loss: sem, target_label and g_sem are needed for a field with semantic classes");
    MNF_REQUIRE(aligned8(loss) && aligned8(target_label) && aligned8(status_word), "pose_loss: loss, labels and the status word must be 8-byte aligned");
    return launch_pose_loss(n_views, rays_per_view, n_classes, rgb, depth, sem, target_rgb, target_depth, target_label, pose, g_rgb, g_depth, g_sem, loss, view_status,
                            status_word, as_stream(stream));
}

extern "C" int mnf_pose_update(const float *g_rays_o, const float *g_rays_d, const float *rays_d, const int64_t *kept_cnts, const int32_t *view_status,
                               const int32_t *skip_dev, int32_t n_views, int32_t rays_per_view, int64_t iteration, const mnf_pose_opts *pose, double *xi, double *adam_m,
                               double *adam_v, int32_t *stalled, double *grad_out, mnf_stream_t stream) {
    if (const int rc = check_pose_opts("pose_update", pose)) return rc;
    MNF_REQUIRE(n_views > 0 && rays_per_view > 0 && (int64_t)n_views * rays_per_view <= 0x7fffffff && iteration >= 0, "pose_update: bad sizes (%d views x %d rays, iteration %lld)",
                n_views, rays_per_view, (long long)iteration);
    MNF_REQUIRE(g_rays_o && g_rays_d && rays_d && xi && adam_m && adam_v && stalled, "pose_update: a null pointer");
    MNF_REQUIRE(aligned8(xi) && aligned8(adam_m) && aligned8(adam_v) && aligned8(grad_out) && aligned8(kept_cnts), "pose_update: float64 and int64 arrays must be 8-byte aligned");
    const PoseUpdateArgs a = {rays_per_view, g_rays_o, g_rays_d, rays_d, kept_cnts, view_status, skip_dev, xi, adam_m, adam_v, stalled, grad_out, iteration,
                              pose->lr_rot, pose->lr_trans, pose->beta1, pose->beta2, pose->eps};
    return launch_pose_update(n_views, a, as_stream(stream));
}

extern "C" int64_t mnf_pose_refine_workspace_bytes(mnf_field_t f, int32_t n_views, int32_t rays_per_view, int64_t max_marched, int64_t max_kept) {
    if (!refine_sizes_ok(f, n_views, rays_per_view, max_marched, max_kept)) return -1;
    return carve_pose(nullptr, f, n_views, rays_per_view, max_marched, max_kept).bytes;
}

extern "C" int64_t mnf_pose_refine_workspace_offset(mnf_field_t f, int32_t n_views, int32_t rays_per_view, int64_t max_marched, int64_t max_kept, int32_t what) {
    if (!refine_sizes_ok(f, n_views, rays_per_view, max_marched, max_kept) || what < 0 || what > MNF_POSE_WS_KEPT) return -1;
    return (int64_t)carve_pose(nullptr, f, n_views, rays_per_view, max_marched, max_kept).off[what];
}

extern "C" int mnf_pose_refine(mnf_field_t f, const uint8_t *binaries, const uint32_t *bitgrid, const float *occs, int32_t res_x, int32_t res_y, int32_t res_z,
                               const float *aabb_host, const uint8_t *images, const void *depths, int32_t depth_is_f16, const void *semantics, int32_t sem_is_u8,
                               int64_t n_images, const int64_t *image_ids, const float *c2w0, float focal, int32_t width, int32_t height, const int64_t *pix_idx,
                               int32_t n_views, int32_t rays_per_view, double *xi, double *adam_m, double *adam_v, int64_t first_iter, int32_t n_iters,
                               const mnf_train_opts *opts, const mnf_pose_opts *pose, double *loss_trace, int32_t *stalled, int64_t *counts_dev, int64_t max_marched,
                               int64_t max_kept, void *workspace, int64_t workspace_bytes, mnf_stream_t stream) {
    MNF_REQUIRE(f && f->params_loaded && opts, "pose_refine: bad handle or options");
    MNF_REQUIRE(opts->struct_size == sizeof(mnf_train_opts), "pose_refine: opts->struct_size is %u, this library's mnf_train_opts has %zu bytes (MNF_INIT)", opts->struct_size,
                sizeof(mnf_train_opts));
    if (const int rc = check_pose_opts("pose_refine", pose)) return rc;
    if (const int rc = check_rays_args("pose_refine", images, depths, semantics, n_images, image_ids, c2w0, focal, width, height, xi, n_views, rays_per_view)) return rc;
    MNF_REQUIRE(max_marched > 0 && max_kept > 0 && opts->render_step_size > 0.f && opts->loss_scale > 0.f && opts->n_levels <= 4,
                "pose_refine: bad sample bounds, step size, loss scale or more than 4 occupancy levels");
    MNF_REQUIRE(first_iter >= 0 && n_iters >= 0 && first_iter + n_iters <= 0xffffffffll, "pose_refine: bad iteration range (%lld + %d)", (long long)first_iter, n_iters);
    MNF_REQUIRE(binaries && occs && aabb_host && adam_m && adam_v && loss_trace && stalled && counts_dev, "pose_refine: a null pointer");
    MNF_REQUIRE(aligned8(adam_m) && aligned8(adam_v) && aligned8(loss_trace) && aligned8(counts_dev) && (!pix_idx || aligned8(pix_idx)),
                "pose_refine: float64 and int64 arrays must be 8-byte aligned");
    const int32_t R = n_views * rays_per_view, C = f->cfg.num_semantic_classes;
    const PoseWs w = carve_pose(workspace, f, n_views, rays_per_view, max_marched, max_kept);
    if (const int rc = check_workspace("pose_refine", workspace, workspace_bytes, w.bytes)) return rc;
    MNF_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 255) == 0, "pose_refine: the workspace must be 256-byte aligned");
    mnf_train_opts t = *opts;      // the render of every iteration: the caller's options, no jitter (the sample set is a constant of each render), no presample
    t.stratified = 0;
    t.presampled = nullptr;
    hipStream_t s = as_stream(stream);
    const int64_t *kept_cnts = train_step_kept_counts(w.step_ws, f, R, max_marched, max_kept);
    for (int32_t it = 0; it < n_iters; ++it) {
        const int64_t iteration = first_iter + it;
        int64_t *counts = counts_dev + 4 * (int64_t)it;
        const PoseRaysArgs ra = {images, depths, semantics, depth_is_f16, sem_is_u8, n_images, image_ids, c2w0, focal, width, height,
                                 pix_idx ? pix_idx : nullptr, xi, n_views, rays_per_view, (uint32_t)iteration, (uint32_t)pose->seed, (uint32_t)(pose->seed >> 32),
                                 w.rays_o, w.rays_d, w.pix, w.rot, w.t_rgb, w.t_dep, w.t_lab};
        if (const int rc = launch_pose_rays(ra, s)) return rc;
        if (const int rc = mnf_train_render_forward(f, binaries, bitgrid, occs, res_x, res_y, res_z, aabb_host, w.rays_o, w.rays_d, R, &t, w.rgb, w.acc, w.depth,
                                                    C > 0 ? w.sem : nullptr, counts, w.skip, max_marched, max_kept, w.step_ws, w.step_bytes, stream))
            return rc;
        if (const int rc = launch_pose_loss(n_views, rays_per_view, C, w.rgb, w.depth, w.sem, w.t_rgb, w.t_dep, w.t_lab, pose, w.g_rgb, w.g_dep, w.g_sem,
                                            loss_trace + (int64_t)it * n_views, w.view_status, counts + 3, s))
            return rc;
        if (const int rc = mnf_train_render_backward_rays(f, R, &t, w.rays_d, w.g_rgb, 3, 1, nullptr, 0, w.g_dep, 1, C > 0 ? w.g_sem : nullptr, C, 1, nullptr, nullptr,
                                                          nullptr, w.g_o, w.g_d, counts, w.skip, max_marched, max_kept, w.step_ws, w.step_bytes, stream))
            return rc;
        const PoseUpdateArgs ua = {rays_per_view, w.g_o, w.g_d, w.rays_d, kept_cnts, w.view_status, w.skip, xi, adam_m, adam_v, stalled, w.grad, iteration,
                                   pose->lr_rot, pose->lr_trans, pose->beta1, pose->beta2, pose->eps};
        if (const int rc = launch_pose_update(n_views, ua, s)) return rc;
    }
    return MNF_OK;
}
