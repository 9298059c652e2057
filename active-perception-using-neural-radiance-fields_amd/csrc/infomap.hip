// Per-pixel predictive-information maps of candidate views on the device (gfx950):
//   mnf_score_view_maps  <- scripts/pipeline.py:727-774 (`ActiveNeRFMapper.probablistic_uncertainty`: the four per-pixel terms that
//                           np.mean collapses at :735 / :746 / :760 / :773), kept per pixel
//
// One pass over the finished probabilistic renders of M members for the same V views of P pixels; score_kernel's arithmetic
// (csrc/render.hip) per pixel, in double from the widened fp32 inputs, k = 2 pi e, members added in order m = 0 .. M - 1:
//   rgb    mean over the three channels of  log(k (sum_m x) / 2 + 1e-4) / 2 - (1 / M) sum_m log(k x_m + 1e-4) / 2     (the / 2 is the
//          reference's, not / M: pipeline.py:733)
//   depth  the same expression on one channel
//   sem    H(mean_m p_m) - mean_m H(p_m), p_m the softmax with the maximum subtracted, H(q) = -sum_k (q_k + 1e-4) log(q_k + 1e-4)
//   occ    B(mean_m a_m) - mean_m B(a_m), B(a) = -(a + 1e-4) log(a + 1e-4) - (1 - a + 1e-4) log(1 - a + 1e-4)
// NaN and inf propagate as they do in numpy.
//
// The work split, the logit staging (member by member) and the reduction of the four sums are view_dev.h's.  The ensemble's class
// probabilities need an accumulator across the members: a row
// of C | 1 doubles per pixel in LDS next to the stage, which only the lane that owns the pixel touches (plain read-modify-writes, no
// barrier of its own; an odd stride in 8-byte units puts the 32 lanes of a ds_read_b64 group on 32 different bank pairs).  No array is
// sized by C or M per lane, so nothing spills to scratch and the same kernel serves 64 members and 1024 classes.  Stage and accumulator
// together take (C | 1) * 12 bytes per pixel and stay within 64 KB per workgroup: the tile shrinks as C grows (256 pixels up to C = 21, 184
// at C = 29, 4 at C = 1024).
//
// Per pixel (3 + 1 + 1 + C) * M * 4 bytes are read, once, and 32 (maps) + 4 (heat8) bytes are written.  The time goes to the double
// exp / log, about 4 M C of them per pixel as score_kernel writes the softmax (exp for the denominator, exp and log per class and member,
// log per class of the ensemble), which is the price of the float64 bar.
//
// Outputs.  maps: the lane's four doubles are 32 contiguous bytes, stored as two 16-byte stores when the base is 16-byte aligned and as
// four 8-byte stores otherwise.  heat8: sat8(((x - lo_k) / (hi_k - lo_k)) * 255.0), every operation rounded on its own (this file is
// compiled with -ffp-contract=off), sat8 as in frames.hip; a pixel's four bytes go out as one aligned 32-bit store.  terms:
// infomap_finish_kernel divides a view's sums.
#include "view_dev.h"

namespace mnf {
namespace {

constexpr int kMapLdsBytes = 65536 - 256;      // stage + accumulator; the rest of 64 KB is left to the reduction's static scratch
constexpr int kMapEntryBytes = 12;             // per class entry: a float of the stage and a double of the accumulator; a tile of >= 4 pixels for C <= 1024
constexpr int kMapTerms = 4;                   // rgb, depth, semantic, occupancy: mnf_score_views' column order

struct HeatRange { double lo[kMapTerms], hi[kMapTerms]; };


__device__ __forceinline__ double binary_entropy(double a) { return -(a + 1e-4) * log(a + 1e-4) - (1.0 - a + 1e-4) * log(1.0 - a + 1e-4); }

__global__ void __launch_bounds__(kViewThreads) infomap_views_kernel(
    const float *__restrict__ rgb_var, const float *__restrict__ depth_var, const float *__restrict__ acc, const float *__restrict__ sem, int M,
    int V, int64_t P, int C, int tp, int64_t tiles, int maps16, HeatRange hr, double *__restrict__ partials,
    double *__restrict__ maps, uint32_t *__restrict__ heat) {
    extern __shared__ double lds[];                                  // p_ens [tp][C | 1] f64, then stage [tp][C | 1] f32
    const int tid = threadIdx.x, v = blockIdx.y, nb = gridDim.x, b = blockIdx.x;
    const int Cs = C | 1;
    double *p_ens = lds + (int64_t)tid * Cs;                         // this lane's row; lanes >= tp never touch it
    float *stage = reinterpret_cast<float *>(lds + (int64_t)tp * Cs);
    const float *row = stage + (int64_t)tid * Cs;
    const double k2pie = 2.0 * 3.14159265358979323846 * 2.71828182845904523536;
    const int64_t VP = (int64_t)V * P;
    const int64_t t0 = tiles * b / nb, t1 = tiles * (b + 1) / nb;
    double s_rgb = 0.0, s_dep = 0.0, s_sem = 0.0, s_occ = 0.0;
    for (int64_t t = t0; t < t1; ++t) {
        const int64_t p0 = t * tp;
        const int np = (int)(P - p0 < tp ? P - p0 : tp);
        const bool own = tid < np;
        const int64_t i = (int64_t)v * P + p0 + tid;                 // this lane's pixel of member 0
        double sum_rgb[3] = {0.0, 0.0, 0.0}, ce_rgb[3] = {0.0, 0.0, 0.0}, sum_dep = 0.0, ce_dep = 0.0, a_ens = 0.0, ce_occ = 0.0, ce_sem = 0.0;
        if (own)
            for (int k = 0; k < C; ++k) p_ens[k] = 0.0;
        for (int m = 0; m < M; ++m) {
            __syncthreads();                                         // the previous piece's rows are read
            stage_rows(stage, sem + (((int64_t)m * V + v) * P + p0) * C, np * C, C, Cs, tid);
            __syncthreads();
            if (own) {
                const int64_t im = i + (int64_t)m * VP;
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) {
                    const double x = (double)rgb_var[3 * im + ch];
                    sum_rgb[ch] += x;
                    ce_rgb[ch] += log(k2pie * x + 1e-4) / 2.0;
                }
                {
                    const double x = (double)depth_var[im];
                    sum_dep += x;
                    ce_dep += log(k2pie * x + 1e-4) / 2.0;
                }
                {
                    const double a = (double)acc[im];
                    a_ens += a;
                    ce_occ += binary_entropy(a);
                }
                double mx = -1e300;
                for (int k = 0; k < C; ++k) mx = fmax(mx, (double)row[k]);
                double den = 0.0;
                for (int k = 0; k < C; ++k) den += exp((double)row[k] - mx);
                double ce = 0.0;
                for (int k = 0; k < C; ++k) {
                    const double pk = exp((double)row[k] - mx) / den;
                    p_ens[k] += pk;
                    ce -= (pk + 1e-4) * log(pk + 1e-4);
                }
                ce_sem += ce;
            }
        }
        if (own) {
            double x_rgb = 0.0;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) x_rgb += log(k2pie * (sum_rgb[ch] / 2.0) + 1e-4) / 2.0 - ce_rgb[ch] / M;
            const double x_dep = log(k2pie * (sum_dep / 2.0) + 1e-4) / 2.0 - ce_dep / M;
            double ent = 0.0;
            for (int k = 0; k < C; ++k) {
                const double pk = p_ens[k] / M;
                ent -= (pk + 1e-4) * log(pk + 1e-4);
            }
            const double x_sem = ent - ce_sem / M;
            const double x_occ = binary_entropy(a_ens / M) - ce_occ / M;
            s_rgb += x_rgb; s_dep += x_dep; s_sem += x_sem; s_occ += x_occ;
            const double px[kMapTerms] = {x_rgb / 3.0, x_dep, x_sem, x_occ};
            if (maps) {
                double *o = maps + 4 * i;
                if (maps16) {
                    reinterpret_cast<double2 *>(o)[0] = make_double2(px[0], px[1]);
                    reinterpret_cast<double2 *>(o)[1] = make_double2(px[2], px[3]);
                } else {
                    o[0] = px[0]; o[1] = px[1]; o[2] = px[2]; o[3] = px[3];
                }
            }
            if (heat) {
                uint32_t w = 0;
#pragma unroll
                for (int k = 0; k < kMapTerms; ++k) w |= (uint32_t)sat8(((px[k] - hr.lo[k]) / (hr.hi[k] - hr.lo[k])) * 255.0) << (8 * k);
                heat[i] = w;
            }
        }
    }
    if (!partials) return;                                           // the same for every lane of the grid
    const double part[kMapTerms] = {s_rgb, s_dep, s_sem, s_occ};
    store_partials(part, partials, v, nb, b, tid);
}

// one wave per view; the means of pipeline.py:735 / :746 / :760 / :773
__global__ void __launch_bounds__(64) infomap_finish_kernel(const double *__restrict__ partials, int nb, int64_t P, double *__restrict__ terms) {
    const int v = blockIdx.x, lane = threadIdx.x;
    double s[kMapTerms];
    sum_partials(partials, v, nb, lane, s);
    if (lane == 0) {
        double *t = terms + (int64_t)v * 4;
        t[0] = s[0] / (3.0 * (double)P);
        t[1] = s[1] / (double)P;
        t[2] = s[2] / (double)P;
        t[3] = s[3] / (double)P;
    }
}

inline bool map_sizes_ok(int32_t n_views, int64_t n_pix, int32_t n_classes) {
    return n_views >= 0 && n_pix > 0 && n_classes > 0 && n_classes <= MNF_SCORE_MAPS_MAX_CLASSES;
}

}  // namespace
}  // namespace mnf

using namespace mnf;

extern "C" int64_t mnf_score_view_maps_workspace_bytes(int32_t n_views, int64_t n_pix, int32_t n_classes) {
    if (!map_sizes_ok(n_views, n_pix, n_classes)) return 0;
    return view_partials_bytes(n_views, view_plan(n_pix, stage_tile_pixels(n_classes, kMapEntryBytes, kMapLdsBytes)).nb, kMapTerms);
}

extern "C" int mnf_score_view_maps(const float *rgb_var, const float *depth_var, const float *acc, const float *sem, int32_t n_members,
                                   int32_t n_views, int64_t n_pix, int32_t n_classes, double *terms, double *maps, uint8_t *heat8,
                                   const double *heat_lo_host, const double *heat_hi_host, void *workspace, int64_t workspace_bytes,
                                   mnf_stream_t stream) {
    MNF_REQUIRE(n_members >= 1, "score_view_maps: n_members must be at least 1 (got %d)", n_members);
    MNF_REQUIRE(n_views >= 0, "score_view_maps: n_views is negative (%d)", n_views);
    MNF_REQUIRE(n_pix > 0, "score_view_maps: n_pix must be positive (got %lld)", (long long)n_pix);
    MNF_REQUIRE(n_classes > 0, "score_view_maps: n_classes must be positive (got %d)", n_classes);
    if (n_members > MNF_SCORE_MAPS_MAX_MEMBERS || n_classes > MNF_SCORE_MAPS_MAX_CLASSES) {
        set_error("score_view_maps: %d members of %d classes are more than the supported %d members of %d classes", n_members, n_classes,
                  MNF_SCORE_MAPS_MAX_MEMBERS, MNF_SCORE_MAPS_MAX_CLASSES);
        return MNF_ERR_UNSUPPORTED;
    }
    if (n_views == 0) return MNF_OK;
    MNF_REQUIRE(terms || maps || heat8, "score_view_maps: terms, maps and heat8 are all null: nothing to compute");
    HeatRange hr = {};
    if (heat8) {
        MNF_REQUIRE(heat_lo_host && heat_hi_host, "score_view_maps: heat8 needs its ranges heat_lo_host and heat_hi_host");
        for (int k = 0; k < kMapTerms; ++k) {
            hr.lo[k] = heat_lo_host[k];
            hr.hi[k] = heat_hi_host[k];
            MNF_REQUIRE(finite_d(hr.lo[k]) && finite_d(hr.hi[k]), "score_view_maps: the heat range of term %d is not finite (%g, %g)", k, hr.lo[k], hr.hi[k]);
            MNF_REQUIRE(hr.hi[k] != hr.lo[k], "score_view_maps: the heat range of term %d is empty (hi == lo == %g)", k, hr.lo[k]);
        }
    }
    MNF_REQUIRE(rgb_var && depth_var && acc && sem, "score_view_maps: null input pointer");
    MNF_REQUIRE(aligned4(rgb_var) && aligned4(depth_var) && aligned4(acc) && aligned4(sem),
                "score_view_maps: the fp32 stacks must be 4-byte aligned");
    MNF_REQUIRE(aligned8(maps), "score_view_maps: maps must be 8-byte aligned");
    MNF_REQUIRE(aligned4(heat8), "score_view_maps: heat8 must be 4-byte aligned");
    MNF_REQUIRE(aligned8(terms), "score_view_maps: terms must be 8-byte aligned");
    MNF_REQUIRE(n_views <= 65535, "score_view_maps: at most 65535 views per call (got %d)", n_views);
    const ViewPlan pl = view_plan(n_pix, stage_tile_pixels(n_classes, kMapEntryBytes, kMapLdsBytes));
    if (terms) {                                                     // the partial sums exist for the per-view means only
        const int64_t need = view_partials_bytes(n_views, pl.nb, kMapTerms);
        MNF_REQUIRE(workspace && aligned8(workspace), "score_view_maps: terms needs an 8-byte aligned workspace");
        MNF_REQUIRE(workspace_bytes >= need, "score_view_maps: workspace too small (%lld < %lld bytes)", (long long)workspace_bytes, (long long)need);
    }
    hipStream_t s = as_stream(stream);
    ProfScope prof("score_view_maps", s);
    const size_t lds = (size_t)pl.tp * (n_classes | 1) * kMapEntryBytes;
    const int maps16 = (reinterpret_cast<uintptr_t>(maps) & 15) == 0;
    double *partials = terms ? reinterpret_cast<double *>(workspace) : nullptr;
    hipLaunchKernelGGL(infomap_views_kernel, dim3(pl.nb, n_views), dim3(kViewThreads), lds, s, rgb_var, depth_var, acc, sem, n_members, n_views, n_pix,
                       n_classes, pl.tp, pl.tiles, maps16, hr, partials, maps, reinterpret_cast<uint32_t *>(heat8));
    int rc = launch_status("infomap_views_kernel");
    if (rc || !terms) return rc;
    hipLaunchKernelGGL(infomap_finish_kernel, dim3(n_views), dim3(64), 0, s, partials, pl.nb, n_pix, terms);
    return launch_status("infomap_finish_kernel");
}
