// Ensemble-disagreement scorer on the device (gfx950):
//   mnf_score_ensemble_views  <- scripts/pipeline.py:861-882 (`ActiveNeRFMapper.trajector_uncertainty`: np.var over the members'
//                                float64 host stacks of rgb and depth, 1 / acc - 1 of member 0, the softmax entropy of member 0's class
//                                logits, each scaled, clipped and averaged per view)
//
// One pass over the finished plain (non-probabilistic) renders of M members for the same V views of P pixels.
//
// The work split, the logit staging and the reduction of the four sums are view_dev.h's; a tile is staged once for every member s < S whose
// logits enter the entropy, so every logit is read from memory once.  The rgb / depth stacks are read once per pass of the two-pass variance
// (mean over the members, then the mean squared deviation: the second pass hits the cache); a sum-of-squares form cancels at depth 5 +- 1e-3
// and is not used.  Per pixel (3 M + M + 1 + S C) * 4 bytes come from HBM.
//
// Everything is double from the widened fp32 inputs: ~2 C double exp / log per pixel and member, which is nothing beside the renders
// (the fp64 transcendentals are software sequences of a few dozen fp64 FMAs at half the fp32 vector rate).  ensemble_finish_kernel scales
// and clips a view's sums; the clips are written as comparisons, so a NaN stays a NaN as it does through np.clip.
#include "view_dev.h"

namespace mnf {
namespace {

constexpr int kEnsPartials = 4;                // sum_p,ch var_m(rgb); sum_p var_m(depth); sum_p clip(1/acc0 - 1); sum_s,p H

// population variance of x[0], x[stride], ..., x[(M - 1) * stride] (np.var, ddof 0), two passes
__device__ __forceinline__ double member_var(const float *__restrict__ x, int64_t stride, int M) {
    double mean = 0.0;
    for (int m = 0; m < M; ++m) mean += (double)x[m * stride];
    mean /= (double)M;
    double ss = 0.0;
    for (int m = 0; m < M; ++m) {
        const double d = (double)x[m * stride] - mean;
        ss += d * d;
    }
    return ss / (double)M;
}

__global__ void __launch_bounds__(kViewThreads) ensemble_views_kernel(
    const float *__restrict__ rgb, const float *__restrict__ depth, const float *__restrict__ acc, const float *__restrict__ sem, int M, int S,
    int V, int64_t P, int C, int tp, int64_t tiles, double *__restrict__ partials) {
    extern __shared__ float stage[];                                 // [tp][C | 1]
    const int tid = threadIdx.x, v = blockIdx.y, nb = gridDim.x, b = blockIdx.x;
    const int Cs = C | 1;
    const int64_t VP = (int64_t)V * P;
    const int64_t t0 = tiles * b / nb, t1 = tiles * (b + 1) / nb;
    double s_rgb = 0.0, s_dep = 0.0, s_acc = 0.0, s_ent = 0.0;
    for (int64_t t = t0; t < t1; ++t) {
        const int64_t p0 = t * tp;
        const int np = (int)(P - p0 < tp ? P - p0 : tp);
        if (tid < np) {
            const int64_t i = (int64_t)v * P + p0 + tid;
#pragma unroll
            for (int k = 0; k < 3; ++k) s_rgb += member_var(rgb + 3 * i + k, 3 * VP, M);
            s_dep += member_var(depth + i, VP, M);
            const double inv = 1.0 / ((double)acc[i] + 1e-4) - 1.0;  // member 0 only (pipeline.py:869)
            s_acc += inv < 0.0 ? 0.0 : (inv > 10000.0 ? 10000.0 : inv);
        }
        for (int s = 0; s < S; ++s) {
            __syncthreads();                                         // the previous piece's rows are read
            stage_rows(stage, sem + (((int64_t)s * V + v) * P + p0) * C, np * C, C, Cs, tid);
            __syncthreads();
            if (tid < np) {
                // H = -sum_k p_k log(p_k + 1e-10), p the float64 softmax with the maximum subtracted (pipeline.py:864-865)
                const float *row = stage + tid * Cs;
                float best = row[0];
                for (int c = 1; c < C; ++c) best = fmaxf(best, row[c]);
                const double mx = (double)best;
                double den = 0.0;
                for (int c = 0; c < C; ++c) den += exp((double)row[c] - mx);
                double h = 0.0;
                for (int c = 0; c < C; ++c) {
                    const double pk = exp((double)row[c] - mx) / den;
                    h -= pk * log(pk + 1e-10);
                }
                s_ent += h;
            }
        }
    }
    const double part[kEnsPartials] = {s_rgb, s_dep, s_acc, s_ent};
    store_partials(part, partials, v, nb, b, tid);
}

__device__ __forceinline__ double clip100(double x) { return x < 0.0 ? 0.0 : (x > 100.0 ? 100.0 : x); }

// one wave per view; pipeline.py:875-882
__global__ void __launch_bounds__(64) ensemble_finish_kernel(const double *__restrict__ partials, int nb, int64_t P, int S, double *__restrict__ terms) {
    const int v = blockIdx.x, lane = threadIdx.x;
    double s[kEnsPartials];
    sum_partials(partials, v, nb, lane, s);
    if (lane == 0) {
        double *t = terms + (int64_t)v * 4;
        t[0] = clip100(s[0] / (3.0 * (double)P) * 4000.0);
        t[1] = clip100(s[1] / (double)P * 50.0);
        t[2] = s[2] / (double)P;
        t[3] = clip100(s[3] / ((double)S * (double)P) * 50.0);
    }
}

inline bool ens_sizes_ok(int32_t n_views, int64_t n_pix, int32_t n_classes) {
    return n_views >= 0 && n_pix > 0 && n_classes > 0 && n_classes <= MNF_SCORE_ENSEMBLE_MAX_CLASSES;
}

}  // namespace
}  // namespace mnf

using namespace mnf;

extern "C" int64_t mnf_score_ensemble_views_workspace_bytes(int32_t n_views, int64_t n_pix, int32_t n_classes) {
    if (!ens_sizes_ok(n_views, n_pix, n_classes)) return 0;
    return view_partials_bytes(n_views, view_plan(n_pix, stage_tile_pixels(n_classes)).nb, kEnsPartials);
}

extern "C" int mnf_score_ensemble_views(const float *rgb, const float *depth, const float *acc, const float *sem, int32_t n_members,
                                        int32_t n_sem_members, int32_t n_views, int64_t n_pix, int32_t n_classes, double *terms,
                                        void *workspace, int64_t workspace_bytes, mnf_stream_t stream) {
    MNF_REQUIRE(n_members >= 1, "score_ensemble_views: n_members must be at least 1 (got %d)", n_members);
    MNF_REQUIRE(n_sem_members >= 1 && n_sem_members <= n_members, "score_ensemble_views: n_sem_members must lie in [1, n_members] (got %d of %d)",
                n_sem_members, n_members);
    MNF_REQUIRE(n_views >= 0, "score_ensemble_views: n_views is negative (%d)", n_views);
    MNF_REQUIRE(n_pix > 0, "score_ensemble_views: n_pix must be positive (got %lld)", (long long)n_pix);
    MNF_REQUIRE(n_classes > 0, "score_ensemble_views: n_classes must be positive (got %d)", n_classes);
    if (n_members > MNF_SCORE_ENSEMBLE_MAX_MEMBERS || n_classes > MNF_SCORE_ENSEMBLE_MAX_CLASSES) {
        set_error("score_ensemble_views: %d members of %d classes are more than the supported %d members of %d classes", n_members, n_classes,
                  MNF_SCORE_ENSEMBLE_MAX_MEMBERS, MNF_SCORE_ENSEMBLE_MAX_CLASSES);
        return MNF_ERR_UNSUPPORTED;
    }
    if (n_views == 0) return MNF_OK;
    MNF_REQUIRE(rgb && depth && acc && sem && terms && workspace, "score_ensemble_views: null pointer");
    MNF_REQUIRE(aligned4(rgb) && aligned4(depth) && aligned4(acc) && aligned4(sem),
                "score_ensemble_views: the fp32 stacks must be 4-byte aligned");
    MNF_REQUIRE(aligned8(workspace) && aligned8(terms),
                "score_ensemble_views: workspace and terms must be 8-byte aligned");
    MNF_REQUIRE(n_views <= 65535, "score_ensemble_views: at most 65535 views per call (got %d)", n_views);
    const ViewPlan pl = view_plan(n_pix, stage_tile_pixels(n_classes));      // a tile of >= 8 pixels for C <= MNF_SCORE_ENSEMBLE_MAX_CLASSES
    const int64_t need = view_partials_bytes(n_views, pl.nb, kEnsPartials);
    MNF_REQUIRE(workspace_bytes >= need, "score_ensemble_views: workspace too small (%lld < %lld bytes)", (long long)workspace_bytes, (long long)need);
    hipStream_t s = as_stream(stream);
    ProfScope prof("score_ensemble_views", s);
    const size_t lds = (size_t)pl.tp * (n_classes | 1) * sizeof(float);
    hipLaunchKernelGGL(ensemble_views_kernel, dim3(pl.nb, n_views), dim3(kViewThreads), lds, s, rgb, depth, acc, sem, n_members, n_sem_members, n_views, n_pix,
                       n_classes, pl.tp, pl.tiles, reinterpret_cast<double *>(workspace));
    int rc = launch_status("ensemble_views_kernel");
    if (rc) return rc;
    hipLaunchKernelGGL(ensemble_finish_kernel, dim3(n_views), dim3(64), 0, s, reinterpret_cast<const double *>(workspace), pl.nb, n_pix, n_sem_members, terms);
    return launch_status("ensemble_finish_kernel");
}
