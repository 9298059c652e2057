// Optimizer step and non-finite guard of the field's flat parameter vectors (pipeline.py:173-178, :520-532).  Nothing here depends on the
// matrix-core operand type: compiled once.
#include <cmath>

#include "field.h"

namespace mnf {
// torch.optim.Adam(lr, betas, eps, weight_decay=0, amsgrad=False) for one element: lerp of the first moment, addcmul of the second, bias-corrected
// step.  Every kernel below updates through these functions, so their arithmetic is the same operation for operation.  (Two halves: adam_kernel stores
// the moments between them, and the order of its stores is part of its instruction stream.)
__device__ __forceinline__ void adam_moments(float gi, float &mi, float &vi, float beta1, float beta2) {
    mi = mi + (gi - mi) * (1.0f - beta1);
    vi = vi * beta2 + (1.0f - beta2) * gi * gi;
}
__device__ __forceinline__ float adam_step(float pi, float mi, float vi, float eps, float step_size, float bc2_sqrt) { return pi - step_size * (mi / (sqrtf(vi) / bc2_sqrt + eps)); }
__device__ __forceinline__ void adam_update(float gi, float &mi, float &vi, float &pi, float beta1, float beta2, float eps, float step_size, float bc2_sqrt) {
    adam_moments(gi, mi, vi, beta1, beta2);
    pi = adam_step(pi, mi, vi, eps, step_size, bc2_sqrt);
}
// NaN as the reference's guard (pipeline.py:520-529), and +-Inf as well: an overflowed fp16 activation gradient shows up
// as Inf, which Adam would turn into NaN parameters one step later
__device__ __forceinline__ int nonfinite(float x) { return !(fabsf(x) <= 3.4028234664e38f); }

// ------------------------------------------------------------------ optimizer step (pipeline.py:173-178, :531)
// One flat parameter vector in a single pass (torch's foreach implementation is six passes over the 25 M table entries).
__global__ void __launch_bounds__(256) adam_kernel(float *__restrict__ p, const float *__restrict__ g, float *__restrict__ m,
                                                   float *__restrict__ v, int64_t n, float beta1, float beta2, float eps,
                                                   float step_size, float bc2_sqrt) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)blockDim.x * gridDim.x) {
        const float gi = g[i];
        float mi = m[i], vi = v[i];
        adam_moments(gi, mi, vi, beta1, beta2);
        m[i] = mi; v[i] = vi;
        p[i] = adam_step(p[i], mi, vi, eps, step_size, bc2_sqrt);
    }
}

// The same update for a training loop that never synchronises with the host: the step count lives on the device and the whole update is
// skipped when `skip` is non-zero (non-finite gradients, pipeline.py:520-529; a step that overflowed its sample bounds or rendered
// no sample, csrc/trainstep.hip).  adam_prepare_kernel advances the count and derives the bias corrections (in double, as the host
// version does); adam_guarded_kernel optionally mirrors the new parameters from `half_from` on into the field handle's fp16 hash
// table, so the per-step fp32 -> fp16 conversion pass over the 25 M entries disappears.
__global__ void adam_prepare_kernel(float *__restrict__ step, const int32_t *__restrict__ skip, float lr, float beta1, float beta2, float *__restrict__ hyper) {
    const bool sk = skip && *skip != 0;
    float st = *step;
    if (!sk) { st += 1.0f; *step = st; }
    const double bc1 = 1.0 - pow((double)beta1, (double)st), bc2 = 1.0 - pow((double)beta2, (double)st);
    hyper[0] = (float)((double)lr / bc1); hyper[1] = (float)sqrt(bc2); hyper[2] = sk ? 1.0f : 0.0f;
}

__global__ void __launch_bounds__(256) adam_guarded_kernel(float *__restrict__ p, const float *__restrict__ g, float *__restrict__ m,
                                                           float *__restrict__ v, int64_t n, float beta1, float beta2, float eps,
                                                           const float *__restrict__ hyper, _Float16 *__restrict__ half_out, int64_t half_from) {
    const float step_size = hyper[0], bc2_sqrt = hyper[1];
    if (hyper[2] != 0.0f) return;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)blockDim.x * gridDim.x) {
        const float gi = g[i];
        float mi = m[i], vi = v[i], pi = p[i];
        adam_update(gi, mi, vi, pi, beta1, beta2, eps, step_size, bc2_sqrt);
        m[i] = mi; v[i] = vi; p[i] = pi;
        if (half_out && i >= half_from) half_out[i - half_from] = (_Float16)pi;
    }
}

// The three parameter vectors of a field in ONE launch each (guard, step counts, update): mnf_field_optimizer_step issued 3 + 3 + 3 launches, most of them ~5 us of nothing.
struct Adam3 {
    float *p[3]; const float *g[3]; float *m[3], *v[3]; float *step[3];
    int64_t n[3];
};
// Both passes over the parameter vectors move 16 bytes per lane and access (one thread = one aligned quad of one vector; the up-to-three elements behind the last
// quad of a vector one by one): with 4-byte accesses the update of the 12.6 M table parameters ran at 2.3 TB/s (167 us of the reference-yaml step's 1.29 ms).
__device__ __forceinline__ bool quad_of(const Adam3 &a, int64_t q, int &k, int64_t &i0) {
    const int64_t q0 = (a.n[0] + 3) >> 2, q1 = (a.n[1] + 3) >> 2, q2 = (a.n[2] + 3) >> 2;
    if (q < q0) { k = 0; i0 = q << 2; return true; }
    if (q < q0 + q1) { k = 1; i0 = (q - q0) << 2; return true; }
    if (q < q0 + q1 + q2) { k = 2; i0 = (q - q0 - q1) << 2; return true; }
    return false;
}
__device__ __forceinline__ bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
__global__ void __launch_bounds__(256) count_nan3_kernel(const Adam3 a, int32_t *__restrict__ count) {
    int local = 0;
    const int64_t quads = ((a.n[0] + 3) >> 2) + ((a.n[1] + 3) >> 2) + ((a.n[2] + 3) >> 2);
    const int64_t stride = (int64_t)blockDim.x * gridDim.x;
    // four quads per trip, their loads issued together (one 16-byte load in flight per thread read the 50 MB of gradients at 2.3 TB/s)
    for (int64_t q0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q0 < quads; q0 += 4 * stride) {
        float4 x[4];
        bool fast[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t q = q0 + u * stride;
            int k = 0; int64_t i0 = 0;
            const bool in = q < quads && quad_of(a, q, k, i0);
            const float *g = a.g[k] + i0;
            fast[u] = in && i0 + 4 <= a.n[k] && aligned16(g);
            x[u] = fast[u] ? *reinterpret_cast<const float4 *>(g) : float4{0.f, 0.f, 0.f, 0.f};
            if (in && !fast[u])
                for (int64_t i = i0; i < a.n[k] && i < i0 + 4; ++i) local += nonfinite(a.g[k][i]);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
            local += nonfinite(x[u].x) + nonfinite(x[u].y) + nonfinite(x[u].z) + nonfinite(x[u].w);
    }
    if (__ballot(local != 0) != 0ull && local) atomicAdd(count, local);
}
__global__ void adam_prepare3_kernel(const Adam3 a, const int32_t *__restrict__ skip, float lr, float beta1, float beta2, float *__restrict__ hyper,
                                     const int64_t *__restrict__ counts, long long *__restrict__ report) {
    const int k = threadIdx.x;
    // the step's report to the host, written straight into pinned host memory: the train step's four counters and its FINAL skip flag (this launch runs behind
    // the non-finite count).  Two device-to-host copies did this before; each cost the stream ~5 us of copy plus ~18 us of bubble around it.
    if (report && k >= 3 && k < 8) {
        report[k - 3] = k < 7 ? (counts ? (long long)counts[k - 3] : 0ll) : (long long)(skip ? *skip : 0);
        __threadfence_system();
    }
    if (k >= 3) return;
    const bool sk = skip && *skip != 0;      // (adam_prepare_kernel's body per vector: through a shared function the compiler drops the second read of *skip)
    float st = *a.step[k];
    if (!sk) { st += 1.0f; *a.step[k] = st; }
    const double bc1 = 1.0 - pow((double)beta1, (double)st), bc2 = 1.0 - pow((double)beta2, (double)st);
    hyper[4 * k] = (float)((double)lr / bc1); hyper[4 * k + 1] = (float)sqrt(bc2); hyper[4 * k + 2] = sk ? 1.0f : 0.0f;
}
__global__ void __launch_bounds__(256) adam_guarded3_kernel(const Adam3 a, float beta1, float beta2, float eps, const float *__restrict__ hyper,
                                                            _Float16 *__restrict__ half_out, int64_t half_from) {
    if (hyper[2] != 0.0f) return;
    const int64_t quads = ((a.n[0] + 3) >> 2) + ((a.n[1] + 3) >> 2) + ((a.n[2] + 3) >> 2);
    auto one = [&](float gi, float &mi, float &vi, float &pi, float step_size, float bc2_sqrt) { adam_update(gi, mi, vi, pi, beta1, beta2, eps, step_size, bc2_sqrt); };
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < quads; q += (int64_t)blockDim.x * gridDim.x) {
        int k; int64_t i0;
        quad_of(a, q, k, i0);
        const float step_size = hyper[4 * k], bc2_sqrt = hyper[4 * k + 1];
        const bool mirror = k == 0 && half_out && i0 >= half_from;
        if (i0 + 4 <= a.n[k] && aligned16(a.g[k] + i0) && aligned16(a.m[k] + i0) && aligned16(a.v[k] + i0) && aligned16(a.p[k] + i0)) {
            const float4 g = *reinterpret_cast<const float4 *>(a.g[k] + i0);
            float4 m = *reinterpret_cast<const float4 *>(a.m[k] + i0), v = *reinterpret_cast<const float4 *>(a.v[k] + i0), p = *reinterpret_cast<const float4 *>(a.p[k] + i0);
            one(g.x, m.x, v.x, p.x, step_size, bc2_sqrt); one(g.y, m.y, v.y, p.y, step_size, bc2_sqrt);
            one(g.z, m.z, v.z, p.z, step_size, bc2_sqrt); one(g.w, m.w, v.w, p.w, step_size, bc2_sqrt);
            *reinterpret_cast<float4 *>(a.m[k] + i0) = m; *reinterpret_cast<float4 *>(a.v[k] + i0) = v; *reinterpret_cast<float4 *>(a.p[k] + i0) = p;
            if (k == 0 && half_out && i0 < half_from && i0 + 4 > half_from) {      // the quad the mirror starts inside
                const float pe[4] = {p.x, p.y, p.z, p.w};
                for (int e = 0; e < 4; ++e) if (i0 + e >= half_from) half_out[i0 + e - half_from] = (_Float16)pe[e];
            }
            if (mirror) {
                _Float16 *h = half_out + (i0 - half_from);
                if ((reinterpret_cast<uintptr_t>(h) & 7) == 0) {
                    typedef _Float16 h4 __attribute__((ext_vector_type(4)));
                    h4 o; o[0] = (_Float16)p.x; o[1] = (_Float16)p.y; o[2] = (_Float16)p.z; o[3] = (_Float16)p.w;
                    *reinterpret_cast<h4 *>(h) = o;
                } else { h[0] = (_Float16)p.x; h[1] = (_Float16)p.y; h[2] = (_Float16)p.z; h[3] = (_Float16)p.w; }
            }
        } else {
            for (int64_t i = i0; i < a.n[k] && i < i0 + 4; ++i) {
                float mi = a.m[k][i], vi = a.v[k][i], pi = a.p[k][i];
                one(a.g[k][i], mi, vi, pi, step_size, bc2_sqrt);
                a.m[k][i] = mi; a.v[k][i] = vi; a.p[k][i] = pi;
                if (k == 0 && half_out && i >= half_from) half_out[i - half_from] = (_Float16)pi;
            }
        }
    }
}

__global__ void __launch_bounds__(256) count_nan_kernel(const float *__restrict__ g, int64_t n, int32_t *__restrict__ count) {
    int local = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)blockDim.x * gridDim.x) local += nonfinite(g[i]);
    if (__ballot(local != 0) != 0ull && local) atomicAdd(count, local);
}
}  // namespace mnf

using namespace mnf;

extern "C" int mnf_adam_step(float *params, const float *grads, float *exp_avg, float *exp_avg_sq, int64_t n, float lr, float beta1,
                             float beta2, float eps, int32_t step, mnf_stream_t stream) {
    if (n == 0) return MNF_OK;
    MNF_REQUIRE(params && grads && exp_avg && exp_avg_sq && step >= 1, "adam_step: bad arguments");
    const double bc1 = 1.0 - std::pow((double)beta1, (double)step), bc2 = 1.0 - std::pow((double)beta2, (double)step);
    const int64_t blocks = ceil_div(n, 256 * 4);
    hipLaunchKernelGGL(adam_kernel, dim3((unsigned)(blocks < 8192 ? (blocks < 1 ? 1 : blocks) : 8192)), dim3(256), 0, as_stream(stream), params,
                       grads, exp_avg, exp_avg_sq, n, beta1, beta2, eps, (float)((double)lr / bc1), (float)std::sqrt(bc2));
    return launch_status("adam_kernel");
}

extern "C" int mnf_adam_step_guarded(float *params, const float *grads, float *exp_avg, float *exp_avg_sq, int64_t n, float lr, float beta1,
                                     float beta2, float eps, float *step_dev, const int32_t *skip_dev, float *hyper_dev, void *half_out,
                                     int64_t half_from, mnf_stream_t stream) {
    if (n == 0) return MNF_OK;
    MNF_REQUIRE(params && grads && exp_avg && exp_avg_sq && step_dev && hyper_dev, "adam_step_guarded: bad arguments");
    MNF_REQUIRE(!half_out || (half_from >= 0 && half_from <= n), "adam_step_guarded: bad fp16 mirror range");
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(adam_prepare_kernel, dim3(1), dim3(1), 0, s, step_dev, skip_dev, lr, beta1, beta2, hyper_dev);
    const int64_t blocks = ceil_div(n, 256 * 4);
    hipLaunchKernelGGL(adam_guarded_kernel, dim3((unsigned)(blocks < 8192 ? (blocks < 1 ? 1 : blocks) : 8192)), dim3(256), 0, s, params, grads, exp_avg,
                       exp_avg_sq, n, beta1, beta2, eps, (const float *)hyper_dev, reinterpret_cast<_Float16 *>(half_out), half_from);
    return launch_status("adam_guarded_kernel");
}

// pipeline.py:520-532 for one model as ONE call: the non-finite-gradient guard over the three parameter vectors, the three Adam updates
// (skipped on the device when the flag is raised) with the fp16 table mirror, and the handle's MLP fragments re-derived.
static int optimizer_step_impl(mnf_field_t f, float *const *params_host, const float *const *grads_host, float *const *exp_avg_host,
                               float *const *exp_avg_sq_host, float *const *step_dev_host, float lr, float beta1, float beta2, float eps,
                               int32_t *skip_dev, int32_t count_nonfinite, float *hyper_dev, const int64_t *counts_dev, int64_t *report_host, mnf_stream_t stream) {
    MNF_REQUIRE(f && params_host && grads_host && exp_avg_host && exp_avg_sq_host && step_dev_host && hyper_dev, "field_optimizer_step: null argument");
    MNF_REQUIRE(f->params_loaded, "field_optimizer_step: the handle holds no parameters yet (mnf_field_set_params)");
    const int64_t n[3] = {f->n_base, f->n_head, f->n_sem};
    Adam3 a;
    for (int k = 0; k < 3; ++k) {
        MNF_REQUIRE(n[k] == 0 || (params_host[k] && grads_host[k] && exp_avg_host[k] && exp_avg_sq_host[k] && step_dev_host[k]), "field_optimizer_step: null pointer");
        a.p[k] = params_host[k]; a.g[k] = grads_host[k]; a.m[k] = exp_avg_host[k]; a.v[k] = exp_avg_sq_host[k]; a.step[k] = step_dev_host[k]; a.n[k] = n[k];
    }
    MNF_REQUIRE(n[0] > 0 && n[1] > 0 && n[2] > 0, "field_optimizer_step: empty parameter vector");
    hipStream_t s = as_stream(stream);
    const int64_t total = n[0] + n[1] + n[2];
    if (count_nonfinite) {
        MNF_REQUIRE(skip_dev, "field_optimizer_step: counting non-finite gradients needs the skip flag");
        const int64_t blocks = ceil_div(total, 256 * 4 * 4);
        hipLaunchKernelGGL(count_nan3_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, s, a, skip_dev);
    }
    hipLaunchKernelGGL(adam_prepare3_kernel, dim3(1), dim3(64), 0, s, a, (const int32_t *)skip_dev, lr, beta1, beta2, hyper_dev, counts_dev,
                       reinterpret_cast<long long *>(report_host));
    const int64_t blocks = ceil_div(total, 256 * 4 * 2);
    hipLaunchKernelGGL(adam_guarded3_kernel, dim3((unsigned)(blocks < 8192 ? blocks : 8192)), dim3(256), 0, s, a, beta1, beta2, eps, (const float *)hyper_dev,
                       reinterpret_cast<_Float16 *>(f->d_table), (int64_t)f->n_base_mlp);
    int rc = launch_status("adam_guarded3_kernel");
    if (rc) return rc;
    return mnf_field_refresh_weights(f, params_host[0], params_host[1], params_host[2], stream);
}

extern "C" int mnf_field_optimizer_step(mnf_field_t f, float *const *params_host, const float *const *grads_host, float *const *exp_avg_host,
                                        float *const *exp_avg_sq_host, float *const *step_dev_host, float lr, float beta1, float beta2, float eps,
                                        int32_t *skip_dev, int32_t count_nonfinite, float *hyper_dev, mnf_stream_t stream) {
    return optimizer_step_impl(f, params_host, grads_host, exp_avg_host, exp_avg_sq_host, step_dev_host, lr, beta1, beta2, eps, skip_dev, count_nonfinite, hyper_dev,
                               nullptr, nullptr, stream);
}

extern "C" int mnf_field_optimizer_step_report(mnf_field_t f, float *const *params_host, const float *const *grads_host, float *const *exp_avg_host,
                                               float *const *exp_avg_sq_host, float *const *step_dev_host, float lr, float beta1, float beta2, float eps,
                                               int32_t *skip_dev, int32_t count_nonfinite, float *hyper_dev, const int64_t *counts_dev, int64_t *report_host,
                                               mnf_stream_t stream) {
    MNF_REQUIRE(report_host, "field_optimizer_step_report: null report buffer");
    return optimizer_step_impl(f, params_host, grads_host, exp_avg_host, exp_avg_sq_host, step_dev_host, lr, beta1, beta2, eps, skip_dev, count_nonfinite, hyper_dev,
                               counts_dev, report_host, stream);
}

extern "C" int mnf_count_nan(const float *values, int64_t n, int32_t *count, mnf_stream_t stream) {
    if (n == 0) return MNF_OK;
    MNF_REQUIRE(values && count, "count_nan: null pointer");
    const int64_t blocks = ceil_div(n, 256 * 8);
    hipLaunchKernelGGL(count_nan_kernel, dim3((unsigned)(blocks < 4096 ? (blocks < 1 ? 1 : blocks) : 4096)), dim3(256), 0, as_stream(stream),
                       values, n, count);
    return launch_status("count_nan_kernel");
}
