// Candidate-view scoring (scripts/pipeline.py): mnf_score_views, :727-781, the predictive-information terms of finished probabilistic renders; mnf_score_poses,
// :674-781 for one trajectory, poses -> sub-sampled rays -> probabilistic renders of every ensemble member -> mnf_score_views; mnf_score_trajectory, :807-882, the
// same plumbing with plain renders and the ensemble-disagreement scorer (ensemble.hip).
// Build with -ffp-contract=off (score_kernel's float64 sums keep every operation separately rounded, as the reference forms them).
#include <vector>

#include "field.h"
#include "reduce_dev.h"
#include "workspace.h"

namespace mnf {

// ------------------------------------------------------------------ scorer (pipeline.py:727-781), one block of kScoreThreads per view
constexpr int kScoreMaxM = 4;             // ensemble sizes the array-free form of the semantic term is unrolled for (the reference's ensemble has two members)
constexpr int kScoreThreads = 1024;      // 16 waves per view: the 4096 pixels of a view are ~220 double-precision exp / log each; four waves per view left three of four issue slots to their latencies (1.07 ms per 256 views)
template <bool SMALL_M>      // SMALL_M: M <= kScoreMaxM (checked by the host)
__global__ void __launch_bounds__(kScoreThreads) score_kernel(const float *__restrict__ rgb_var, const float *__restrict__ depth_var,
                                                    const float *__restrict__ acc, const float *__restrict__ sem,
                                                    int M, int V, int P, int C, double *__restrict__ terms) {
    __shared__ double s_buf[kScoreThreads / 64];
    const int v = blockIdx.x;
    const double k2pie = 2.0 * 3.14159265358979323846 * 2.71828182845904523536;
    double s_rgb = 0.0, s_dep = 0.0, s_sem = 0.0, s_occ = 0.0;
    for (int p = threadIdx.x; p < P; p += blockDim.x) {
        // rgb / depth: entropy of the summed variance minus mean member entropy (pipeline.py:727-746)
        for (int ch = 0; ch < 3; ++ch) {
            double sum_var = 0.0, mean_ce = 0.0;
            for (int m = 0; m < M; ++m) {
                const double x = rgb_var[(((int64_t)m * V + v) * P + p) * 3 + ch];
                sum_var += x;
                mean_ce += log(k2pie * x + 1e-4) / 2.0;
            }
            s_rgb += log(k2pie * (sum_var / 2.0) + 1e-4) / 2.0 - mean_ce / M;
        }
        {
            double sum_var = 0.0, mean_ce = 0.0;
            for (int m = 0; m < M; ++m) {
                const double x = depth_var[((int64_t)m * V + v) * P + p];
                sum_var += x;
                mean_ce += log(k2pie * x + 1e-4) / 2.0;
            }
            s_dep += log(k2pie * (sum_var / 2.0) + 1e-4) / 2.0 - mean_ce / M;
        }
        // semantics (pipeline.py:748-760)
        if constexpr (SMALL_M) {
            // class by class with the members' max / denominator worked out first: the same sums in the same order as the general form below, without its
            // per-class array (dynamically indexed -> 272 bytes of scratch per lane, which was most of this kernel's time)
            double mx[kScoreMaxM], den[kScoreMaxM], ce[kScoreMaxM];
#pragma unroll
            for (int m = 0; m < kScoreMaxM; ++m) {
                mx[m] = -1e300; den[m] = 0.0; ce[m] = 0.0;
                if (m < M) {
                    const float *lg = sem + (((int64_t)m * V + v) * P + p) * C;
                    for (int k = 0; k < C; ++k) mx[m] = fmax(mx[m], (double)lg[k]);
                    for (int k = 0; k < C; ++k) den[m] += exp((double)lg[k] - mx[m]);
                }
            }
            double ent = 0.0;
            for (int k = 0; k < C; ++k) {
                double pe = 0.0;
#pragma unroll
                for (int m = 0; m < kScoreMaxM; ++m)
                    if (m < M) {
                        const double pk = exp((double)sem[(((int64_t)m * V + v) * P + p) * C + k] - mx[m]) / den[m];
                        pe += pk;
                        ce[m] -= (pk + 1e-4) * log(pk + 1e-4);
                    }
                pe /= M;
                ent -= (pe + 1e-4) * log(pe + 1e-4);
            }
            double mean_ce = 0.0;
#pragma unroll
            for (int m = 0; m < kScoreMaxM; ++m) if (m < M) mean_ce += ce[m];
            s_sem += ent - mean_ce / M;
        } else {
            double p_ens[32];
            for (int k = 0; k < C; ++k) p_ens[k] = 0.0;
            double mean_ce = 0.0;
            for (int m = 0; m < M; ++m) {
                const float *lg = sem + (((int64_t)m * V + v) * P + p) * C;
                double mx = -1e300;
                for (int k = 0; k < C; ++k) mx = fmax(mx, (double)lg[k]);
                double den = 0.0;
                for (int k = 0; k < C; ++k) den += exp((double)lg[k] - mx);
                double ce = 0.0;
                for (int k = 0; k < C; ++k) {
                    const double pk = exp((double)lg[k] - mx) / den;
                    p_ens[k] += pk;
                    ce -= (pk + 1e-4) * log(pk + 1e-4);
                }
                mean_ce += ce;
            }
            double ent = 0.0;
            for (int k = 0; k < C; ++k) { const double pk = p_ens[k] / M; ent -= (pk + 1e-4) * log(pk + 1e-4); }
            s_sem += ent - mean_ce / M;
        }
        // occupancy (pipeline.py:762-773)
        {
            double a_ens = 0.0, mean_ce = 0.0;
            for (int m = 0; m < M; ++m) {
                const double a = acc[((int64_t)m * V + v) * P + p];
                a_ens += a;
                mean_ce += -(a + 1e-4) * log(a + 1e-4) - (1.0 - a + 1e-4) * log(1.0 - a + 1e-4);
            }
            a_ens /= M;
            s_occ += -(a_ens + 1e-4) * log(a_ens + 1e-4) - (1.0 - a_ens + 1e-4) * log(1.0 - a_ens + 1e-4) - mean_ce / M;
        }
    }
    constexpr int kWaves = kScoreThreads / 64;      // (both launches below use kScoreThreads)
    const double t0 = block_sum<kWaves>(s_rgb, s_buf), t1 = block_sum<kWaves>(s_dep, s_buf), t2 = block_sum<kWaves>(s_sem, s_buf),
                 t3 = block_sum<kWaves>(s_occ, s_buf);
    if (threadIdx.x == 0) {
        terms[4 * v + 0] = t0 / (3.0 * P);
        terms[4 * v + 1] = t1 / P;
        terms[4 * v + 2] = t2 / P;
        terms[4 * v + 3] = t3 / P;
    }
}

namespace {

// view groups per member of a scoring call.  FOUR render jobs in flight (the caller's stream + the three shared side streams) is the measured optimum for
// these small views (profiles/r03_hw_queues.txt: 256 views x 2 members 101.1 ms with 4 jobs, 107.0 with 2; 32 views 21.3 against 22.6; more jobs than
// streams: worse): two members -> two halves of the pose list each, one member -> four quarters; one half's marcher runs beside another's field kernel.
// (profiles/r03_split_experiment.txt had two as the optimum: measured when every job still had a stream of its own, see common.h shared_side_stream.)
inline int score_groups(int32_t n_views, int32_t n_members = 1) {
    int g = 4 / (n_members > 0 ? n_members : 1);
    if (g < 1) g = 1;
    return g > n_views ? (n_views > 0 ? n_views : 1) : g;
}
inline int32_t group_lo(int32_t n_views, int g, int G) { return (int32_t)((int64_t)n_views * g / G); }

// A scoring call's workspace.  probabilistic (mnf_score_poses): the stacks hold rgb_var / depth_var / acc / sem, the plain rgb / depth go to per-member scratch planes
struct ScoreWs {
    float *rays_o, *rays_d;                  // [V * P][3]: the sub-sampled rays of every view
    float *wide, *narrow, *acc, *sem;        // member-major stacks [M][V * P] x 3, 1, 1, C: exactly what mnf_score_views / mnf_score_ensemble_views read
    void *ensemble; int64_t ensemble_bytes;  // not probabilistic (mnf_score_trajectory: the stacks hold rgb / depth / acc / sem, no variance is rendered): the ensemble scorer's region
    int64_t bytes;
};

// `jobs` (NULL: size only) receives every (member, view group) as a render job with its rays, its output planes, its 64-byte sample total and its render workspace
ScoreWs carve_score(void *base, int32_t n_members, int32_t n_views, int64_t n_pix, int32_t C, bool probabilistic, std::vector<mnf_render_job> *jobs) {
    ScoreWs w = {};
    Carver c(base);
    const size_t R = (size_t)n_views * n_pix;
    w.rays_o = c.take<float>(R * 3); w.rays_d = c.take<float>(R * 3);
    w.wide = c.take<float>(n_members * R * 3); w.narrow = c.take<float>(n_members * R);
    w.acc = c.take<float>(n_members * R); w.sem = c.take<float>(n_members * R * C);
    const int G = score_groups(n_views, n_members);
    for (int m = 0; m < n_members; ++m) {
        float *rgb = nullptr, *depth = nullptr;
        if (probabilistic) { rgb = c.take<float>(R * 3); depth = c.take<float>(R); }          // outputs the scorer does not read
        for (int g = 0; g < G; ++g) {
            const int64_t r0 = (int64_t)group_lo(n_views, g, G) * n_pix, r1 = (int64_t)group_lo(n_views, g + 1, G) * n_pix;
            mnf_render_job j = {};
            j.struct_size = (uint32_t)sizeof(j);
            j.n_rays = r1 - r0;
            j.total_samples = c.take<int64_t>(8);
            j.workspace_bytes = mnf_render_workspace_bytes(j.n_rays, (int32_t)n_pix);
            j.workspace = c.take((size_t)j.workspace_bytes);
            if (!jobs) continue;
            j.rays_o = w.rays_o + 3 * r0; j.rays_d = w.rays_d + 3 * r0;
            j.rgb = (probabilistic ? rgb : w.wide + (size_t)m * R * 3) + 3 * r0; j.depth = (probabilistic ? depth : w.narrow + (size_t)m * R) + r0;
            j.acc = w.acc + (size_t)m * R + r0; j.sem = w.sem + ((size_t)m * R + r0) * C;
            if (probabilistic) { j.rgb_var = w.wide + ((size_t)m * R + r0) * 3; j.depth_var = w.narrow + (size_t)m * R + r0; }
            jobs->push_back(j);
        }
    }
    w.ensemble_bytes = probabilistic ? 0 : mnf_score_ensemble_views_workspace_bytes(n_views, n_pix, C);
    w.ensemble = c.take((size_t)w.ensemble_bytes);      // (probabilistic: no bytes)
    w.bytes = c.bytes();
    return w;
}

// mnf_score_poses and mnf_score_trajectory: c2w -> the sub-sampled rays of every view -> every member's render as jobs of ONE mnf_render_jobs call -> the scorer
int score_from_poses(const char *what, const mnf_field_t *fields_host, const uint8_t *const *binaries_host, const uint32_t *const *bitgrids_host,
                     int32_t n_members, int32_t res_x, int32_t res_y, int32_t res_z, const float *aabb_host, const float *c2w, int32_t n_views,
                     int32_t width, int32_t height, float focal, const int64_t *pix_idx, int64_t n_pix, const mnf_render_opts *opts, bool probabilistic,
                     double *terms, void *workspace, int64_t workspace_bytes, mnf_stream_t stream) {
    MNF_REQUIRE(fields_host && binaries_host && aabb_host && c2w && opts && terms && workspace && pix_idx, "%s: null pointer", what);
    MNF_REQUIRE(opts->struct_size == sizeof(mnf_render_opts), "%s: opts->struct_size is %u, this library's mnf_render_opts has %zu bytes (MNF_INIT)", what,
                opts->struct_size, sizeof(mnf_render_opts));
    MNF_REQUIRE(n_members >= 1 && n_members <= 16 && n_views >= 1 && n_pix >= 1, "%s: bad sizes", what);
    const int C = fields_host[0]->cfg.num_semantic_classes;
    for (int m = 1; m < n_members; ++m) MNF_REQUIRE(fields_host[m]->cfg.num_semantic_classes == C, "%s: members disagree on the class count", what);
    // every (member, half of the pose list) is a render job of its own: they advance side by side (mnf_render_jobs)
    std::vector<mnf_render_job> jobs;
    const ScoreWs w = carve_score(workspace, n_members, n_views, n_pix, C, probabilistic, &jobs);
    if (const int rc = check_workspace(what, workspace, workspace_bytes, w.bytes)) return rc;
    for (size_t i = 0, G = jobs.size() / n_members; i < jobs.size(); ++i) {
        jobs[i].field = fields_host[i / G]; jobs[i].binaries = binaries_host[i / G]; jobs[i].bitgrid = bitgrids_host ? bitgrids_host[i / G] : nullptr;
    }
    if (const int rc = mnf_generate_rays(c2w, n_views, width, height, focal, pix_idx, n_pix, w.rays_o, w.rays_d, stream)) return rc;
    mnf_render_opts ro = *opts;
    ro.probabilistic = probabilistic ? 1 : 0; ro.rays_per_view = (int32_t)n_pix; ro.bitgrid = nullptr;      // (the caller's view_order, if any, applies to every view)
    if (!probabilistic) ro.render_bkgd[0] = ro.render_bkgd[1] = ro.render_bkgd[2] = 0.f;
    if (const int rc = mnf_render_jobs(jobs.data(), (int32_t)jobs.size(), res_x, res_y, res_z, aabb_host, &ro, stream)) return rc;
    if (probabilistic) return mnf_score_views(w.wide, w.narrow, w.acc, w.sem, n_members, n_views, (int32_t)n_pix, C, terms, stream);
    return mnf_score_ensemble_views(w.wide, w.narrow, w.acc, w.sem, n_members, 1, n_views, n_pix, C, terms, w.ensemble, w.ensemble_bytes, stream);
}

}  // namespace
}  // namespace mnf

using namespace mnf;

extern "C" int mnf_score_views(const float *rgb_var, const float *depth_var, const float *acc, const float *sem,
                               int32_t n_members, int32_t n_views, int32_t n_pix, int32_t n_classes, double *terms, mnf_stream_t stream) {
    MNF_REQUIRE(n_members >= 1 && n_views >= 0 && n_pix > 0 && n_classes >= 1 && n_classes <= 32, "score_views: bad sizes");
    if (n_views == 0) return MNF_OK;
    MNF_REQUIRE(rgb_var && depth_var && acc && sem && terms, "score_views: null pointer");
    if (n_members <= kScoreMaxM)
        hipLaunchKernelGGL(score_kernel<true>, dim3(n_views), dim3(kScoreThreads), 0, as_stream(stream), rgb_var, depth_var, acc, sem, n_members, n_views,
                           n_pix, n_classes, terms);
    else
        hipLaunchKernelGGL(score_kernel<false>, dim3(n_views), dim3(kScoreThreads), 0, as_stream(stream), rgb_var, depth_var, acc, sem, n_members, n_views,
                           n_pix, n_classes, terms);
    return launch_status("score_kernel");
}

extern "C" int64_t mnf_score_poses_workspace_bytes(int32_t n_members, int32_t n_views, int32_t n_pix, int32_t n_classes) {
    if (n_members <= 0 || n_views <= 0 || n_pix <= 0 || n_classes <= 0) return -1;
    return carve_score(nullptr, n_members, n_views, n_pix, n_classes, true, nullptr).bytes;
}

extern "C" int mnf_score_poses(const mnf_field_t *fields_host, const uint8_t *const *binaries_host, const uint32_t *const *bitgrids_host,
                               int32_t n_members, int32_t res_x, int32_t res_y, int32_t res_z, const float *aabb_host, const float *c2w,
                               int32_t n_views, int32_t width, int32_t height, float focal, const int64_t *pix_idx, int64_t n_pix,
                               const mnf_render_opts *opts, double *terms, void *workspace, int64_t workspace_bytes, mnf_stream_t stream) {
    return score_from_poses("score_poses", fields_host, binaries_host, bitgrids_host, n_members, res_x, res_y, res_z, aabb_host, c2w, n_views, width, height, focal,
                            pix_idx, n_pix, opts, true, terms, workspace, workspace_bytes, stream);
}

extern "C" int64_t mnf_score_trajectory_workspace_bytes(int32_t n_members, int32_t n_views, int32_t n_pix, int32_t n_classes) {
    if (n_members <= 0 || n_views <= 0 || n_pix <= 0 || n_classes <= 0) return -1;
    return carve_score(nullptr, n_members, n_views, n_pix, n_classes, false, nullptr).bytes;
}

extern "C" int mnf_score_trajectory(const mnf_field_t *fields_host, const uint8_t *const *binaries_host, const uint32_t *const *bitgrids_host,
                                    int32_t n_members, int32_t res_x, int32_t res_y, int32_t res_z, const float *aabb_host, const float *c2w,
                                    int32_t n_views, int32_t width, int32_t height, float focal, const int64_t *pix_idx, int64_t n_pix,
                                    const mnf_render_opts *opts, double *terms, void *workspace, int64_t workspace_bytes, mnf_stream_t stream) {
    return score_from_poses("score_trajectory", fields_host, binaries_host, bitgrids_host, n_members, res_x, res_y, res_z, aabb_host, c2w, n_views, width, height,
                            focal, pix_idx, n_pix, opts, false, terms, workspace, workspace_bytes, stream);
}
