// Held-out view evaluation on the device (gfx950):
//   mnf_eval_views  <- scripts/pipeline.py:550-613 (per test image: F.cross_entropy on the [H*W, C] logits, F.mse_loss on rgb and
//                      depth, PSNR, each read back with .item(), every plane copied to the host) and :1011 (np.argmax over a float64
//                      [H, W, C] host stack for the label image)
//
// One pass over the finished renders of V views of P pixels.  Ground truth is read straight from the dataset's storage (u8 images,
// f32 / f16 depths, i64 / u8 labels: the two layouts of pixel_dev.h); no fp32 ground-truth image is written.
//
// The work split, the logit staging and the reduction of the six sums are view_dev.h's.  Per pixel (3 + 1 + C) * 4 bytes of render and 15
// (u8 / f32 / i64) or 6 (u8 / f16 / u8) bytes of ground truth are read, once.  The confusion matrix is counted with integer atomics (an LDS
// histogram per workgroup for C <= 64, flushed with one 64-bit global atomic per non-zero cell; straight to global above that).
#include "pixel_dev.h"
#include "view_dev.h"

namespace mnf {
namespace {

constexpr int kEvalHistClasses = 64;          // C <= 64: per-workgroup LDS histogram (64 * 64 * 4 B = 16 KB; + kStageBytes + the reduction scratch < 64 KB)
constexpr int kEvalPartials = 6;              // rgb squared error, depth squared error, cross-entropy, correct, valid, invalid

__global__ void __launch_bounds__(kViewThreads) eval_views_kernel(
    const float *__restrict__ rgb, const float *__restrict__ depth, const float *__restrict__ sem, int64_t P, int C, int tp, int64_t tiles,
    const uint8_t *__restrict__ images, const void *__restrict__ depths, int depth_f16, const void *__restrict__ sems, int sem_u8,
    int64_t pixels_per_image, const int64_t *__restrict__ image_ids, const int64_t *__restrict__ pix_idx, double *__restrict__ partials,
    unsigned long long *__restrict__ confusion, uint8_t *__restrict__ pred_labels) {
    extern __shared__ float stage[];                                 // [tp][C | 1]
    __shared__ unsigned int hist[kEvalHistClasses * kEvalHistClasses];
    const int tid = threadIdx.x, v = blockIdx.y, nb = gridDim.x, b = blockIdx.x;
    const int Cs = C | 1;
    const bool lds_hist = confusion && C <= kEvalHistClasses;
    if (lds_hist) {
        for (int i = tid; i < C * C; i += kViewThreads) hist[i] = 0u;
    }
    const int64_t gt_base = image_ids[v] * pixels_per_image;
    const int64_t t0 = tiles * b / nb, t1 = tiles * (b + 1) / nb;
    double s_rgb = 0.0, s_dep = 0.0, s_ce = 0.0, n_ok = 0.0, n_valid = 0.0, n_bad = 0.0;
    for (int64_t t = t0; t < t1; ++t) {
        const int64_t p0 = t * tp;
        const int np = (int)(P - p0 < tp ? P - p0 : tp);
        __syncthreads();                                             // the previous tile's rows are read; the histogram is zeroed
        stage_rows(stage, sem + ((int64_t)v * P + p0) * C, np * C, C, Cs, tid);
        __syncthreads();
        if (tid < np) {
            const int64_t p = p0 + tid, i = (int64_t)v * P + p;
            const int64_t g = gt_base + (pix_idx ? pix_idx[p] : p);
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const float gt = unit_u8(images[3 * g + k]);
                const double d = (double)rgb[3 * i + k] - (double)gt;
                s_rgb += d * d;
            }
            const float gd = load_depth(depths, depth_f16, g);
            const double dd = (double)depth[i] - (double)gd;
            s_dep += dd * dd;
            const int64_t label = load_label(sems, sem_u8, g);
            const float *row = stage + tid * Cs;
            float best;
            const int arg = first_argmax(row, C, &best);
            if (pred_labels) pred_labels[i] = (uint8_t)arg;
            if (label >= 0 && label < C) {
                const double m = (double)best;
                double se = 0.0;
                for (int c = 0; c < C; ++c) se += exp((double)row[c] - m);
                s_ce += (m + log(se)) - (double)row[label];
                n_valid += 1.0;
                n_ok += arg == (int)label ? 1.0 : 0.0;
                if (lds_hist) atomicAdd(&hist[(int)label * C + arg], 1u);
                else if (confusion) atomicAdd(&confusion[label * C + arg], 1ull);
            } else {
                n_bad += 1.0;
            }
        }
    }
    const double part[kEvalPartials] = {s_rgb, s_dep, s_ce, n_ok, n_valid, n_bad};
    store_partials(part, partials, v, nb, b, tid);                   // its barrier also: every histogram count of this workgroup is in
    if (lds_hist) {
        for (int i = tid; i < C * C; i += kViewThreads) {
            const unsigned int n = hist[i];
            if (n) atomicAdd(&confusion[i], (unsigned long long)n);
        }
    }
}

// one wave per view
__global__ void __launch_bounds__(64) eval_finish_kernel(const double *__restrict__ partials, int nb, int64_t P, double *__restrict__ metrics) {
    const int v = blockIdx.x, lane = threadIdx.x;
    double s[kEvalPartials];
    sum_partials(partials, v, nb, lane, s);
    if (lane == 0) {
        double *m = metrics + (int64_t)v * 8;
        const double mse = s[0] / (double)(3 * P);
        const double nan = __longlong_as_double(0x7ff8000000000000ll);
        m[0] = mse;
        m[1] = -10.0 * log(mse) / log(10.0);                         // pipeline.py:601; +inf at mse 0
        m[2] = s[1] / (double)P;
        m[3] = s[4] > 0.0 ? s[2] / s[4] : nan;
        m[4] = s[4] > 0.0 ? s[3] / s[4] : nan;
        m[5] = s[4];
        m[6] = s[5];
        m[7] = 0.0;
    }
}

}  // namespace
}  // namespace mnf

using namespace mnf;

extern "C" int64_t mnf_eval_views_workspace_bytes(int32_t n_views, int64_t n_pix, int32_t n_classes) {
    if (n_views < 0 || n_pix <= 0 || n_classes <= 0 || stage_tile_pixels(n_classes) < 1) return 0;
    return view_partials_bytes(n_views, view_plan(n_pix, stage_tile_pixels(n_classes)).nb, kEvalPartials);
}

extern "C" int mnf_eval_views(const float *rgb, const float *depth, const float *sem, int32_t n_views, int64_t n_pix, int32_t n_classes,
                              const uint8_t *gt_images, const void *gt_depths, int32_t depth_is_f16, const void *gt_semantics, int32_t sem_is_u8,
                              int64_t pixels_per_image, const int64_t *image_ids, const int64_t *pix_idx,
                              double *metrics, int64_t *confusion, uint8_t *pred_labels,
                              void *workspace, int64_t workspace_bytes, mnf_stream_t stream) {
    MNF_REQUIRE(n_views >= 0, "eval_views: n_views is negative (%d)", n_views);
    MNF_REQUIRE(n_pix > 0, "eval_views: n_pix must be positive (got %lld)", (long long)n_pix);
    MNF_REQUIRE(n_classes > 0, "eval_views: n_classes must be positive (got %d)", n_classes);
    MNF_REQUIRE(!pred_labels || n_classes <= 256, "eval_views: pred_labels holds uint8 class ids and needs n_classes <= 256 (got %d)", n_classes);
    MNF_REQUIRE(pixels_per_image > 0, "eval_views: pixels_per_image must be positive (got %lld)", (long long)pixels_per_image);
    MNF_REQUIRE(pix_idx || n_pix <= pixels_per_image, "eval_views: n_pix (%lld) exceeds pixels_per_image (%lld) with no pix_idx", (long long)n_pix,
                (long long)pixels_per_image);
    if (n_views == 0) return MNF_OK;
    MNF_REQUIRE(rgb, "eval_views: rgb is null");
    MNF_REQUIRE(depth, "eval_views: depth is null");
    MNF_REQUIRE(sem, "eval_views: sem is null");
    MNF_REQUIRE(gt_images, "eval_views: gt_images is null");
    MNF_REQUIRE(gt_depths, "eval_views: gt_depths is null");
    MNF_REQUIRE(gt_semantics, "eval_views: gt_semantics is null");
    MNF_REQUIRE(image_ids, "eval_views: image_ids is null");
    MNF_REQUIRE(metrics, "eval_views: metrics is null");
    MNF_REQUIRE(workspace, "eval_views: workspace is null");
    MNF_REQUIRE(aligned8(workspace), "eval_views: workspace must be 8-byte aligned");
    const int tp = stage_tile_pixels(n_classes);
    if (tp < 1) {
        set_error("eval_views: n_classes = %d is more than one LDS tile holds (%d)", n_classes, kStageBytes / 4 - 1);
        return MNF_ERR_UNSUPPORTED;
    }
    const ViewPlan pl = view_plan(n_pix, tp);
    const int64_t need = view_partials_bytes(n_views, pl.nb, kEvalPartials);
    MNF_REQUIRE(workspace_bytes >= need, "eval_views: workspace too small (%lld < %lld bytes)", (long long)workspace_bytes, (long long)need);
    MNF_REQUIRE(n_views <= 65535, "eval_views: at most 65535 views per call (got %d)", n_views);
    hipStream_t s = as_stream(stream);
    ProfScope prof("eval_views", s);
    if (confusion) MNF_HIP(hipMemsetAsync(confusion, 0, (size_t)n_classes * n_classes * sizeof(int64_t), s));    // written, not accumulated into
    const size_t lds = (size_t)pl.tp * (n_classes | 1) * sizeof(float);
    hipLaunchKernelGGL(eval_views_kernel, dim3(pl.nb, n_views), dim3(kViewThreads), lds, s, rgb, depth, sem, n_pix, n_classes, pl.tp, pl.tiles, gt_images, gt_depths, depth_is_f16, gt_semantics, sem_is_u8, pixels_per_image, image_ids, pix_idx,
                       reinterpret_cast<double *>(workspace), reinterpret_cast<unsigned long long *>(confusion), pred_labels);
    int rc = launch_status("eval_views_kernel");
    if (rc) return rc;
    hipLaunchKernelGGL(eval_finish_kernel, dim3(n_views), dim3(64), 0, s, reinterpret_cast<const double *>(workspace), pl.nb, n_pix, metrics);
    return launch_status("eval_finish_kernel");
}
