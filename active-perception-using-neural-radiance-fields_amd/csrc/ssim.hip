// Structural similarity of finished renders on the device (gfx950):
//   mnf_ssim_views  <- scripts/pipeline.py:550-613 (the evaluation block: PSNR is there, SSIM is the number NeRF papers print next to it;
//                      the reference imports skimage at :20, whose structural_similarity(gaussian_weights=True, sigma=1.5,
//                      use_sample_covariance=False, data_range=L, channel_axis=-1) this restates over the valid windows)
//
// Per view of H x W pixels of K channels and per channel, in double from the widened fp32 inputs: the five planes x, y, x x, y y, x y are
// filtered with the separable 11-tap Gaussian g (sigma 1.5, normalised), rows (along W) first, then columns, taps added in index order, no
// padding: (H - 10) x (W - 10) window centres.  vx = E[xx] - mx mx, vy likewise, cxy = E[xy] - mx my,
//   S = ((2 mx my + C1) (2 cxy + C2)) / ((mx mx + my my + C1) (vx + vy + C2)),  C1 = (k1 L)^2, C2 = (k2 L)^2.
// map = the mean of S over the channels, ssim = the mean of S over centres and channels.  This file is compiled with -ffp-contract=off:
// without FMA contraction 2 (m m) and m m + m m are the same double, so identical images give exactly 1.0 at every centre.
//
// Work split.  The first pass of this library that needs a pixel's NEIGHBOURHOOD: view_dev.h walks a 1-D pixel run one pixel per lane; here a
// view's centres are cut into 2-D tiles of kTileH x kTileW = 8 x 32 centres, one centre per lane of a 256-lane workgroup, lane t = centre
// (t / 32, t % 32).  A view's tiles (row-major) are cut into nb contiguous runs exactly as view_plan cuts pixel tiles; grid (nb, V).  The
// plan depends on H, W (and nothing else), so a view's bits do not depend on n_views or on its position in the call.
// Per tile:
//   stage    the (th + 10) x (tw + 10) x K patch of both images goes to LDS as floats, de-interleaved into K planes of row stride 42.  A patch
//            row is one contiguous piece of the image: one wave per row takes it as stage_rows takes a tile (scalar loads up to the first
//            16-byte boundary of the ADDRESS, 16-byte loads, scalar tail), so nothing outside the planes is read.  A u8 target is converted
//            here with unit_u8 (pixel_dev.h).
//   row pass per channel: lane j of 18 x 32 jobs filters 11 consecutive floats of one patch row of x and of y (stride-1 ds_read_b32 across
//            the 32 lanes of a group: conflict-free) into the five doubles of planes[5][18][32].
//   column pass per channel: lane t adds 11 rows of each plane; the 32 lanes of a ds_read_b64 group read 32 consecutive doubles = 256
//            bytes = the 64 banks once: conflict-free.
// LDS: 2 * K * 18 * 42 * 4 (24,192 B at K = 4) + 5 * 18 * 32 * 8 (23,040 B) + the reduction's 32 B.  No array is sized by H or W.
// Sums: per lane over its centres and channels in double, then view_dev.h's store_partials / sum_partials; ssim_finish_kernel divides.  No
// floating-point atomic.
//
// Per pixel 2 * 4 K bytes (f32 target) or 4 K + 3 bytes (u8) are read from memory, (18 * 42) / (8 * 32) = 2.95 times over through the halo
// (from L2 after the first touch), and 8 bytes of map are written.  Per centre and channel the two passes take 2.25 * 11 * 13 + 11 * 10
// double operations and 2.25 * 22 + 55 LDS reads: the double arithmetic and the LDS, not the memory, bound the kernel.
#include <cmath>

#include "pixel_dev.h"
#include "view_dev.h"

namespace mnf {
namespace {

constexpr int kSsimTaps = MNF_SSIM_WINDOW;                      // 11 taps, sigma MNF_SSIM_SIGMA = 1.5
constexpr int kSsimHalo = kSsimTaps - 1;
constexpr int kTileH = 8, kTileW = 32;                          // centres per tile: kTileH * kTileW == kViewThreads
constexpr int kPatchH = kTileH + kSsimHalo, kPatchW = kTileW + kSsimHalo;
constexpr int kSsimPlanes = 5;                                  // E[x], E[y], E[xx], E[yy], E[xy]
static_assert(kTileH * kTileW == kViewThreads, "one centre per lane");
static_assert(kPatchW <= 64, "one wave stages a patch row");

struct SsimParams { double g[kSsimTaps]; double c1, c2; };

// One patch row of image `img`: its n = pw * K contiguous elements at `src` into dst[c * kPatchH * kPatchW + px] for element px * K + c.
// Called by the 64 lanes of one wave; vector loads between the first and the last 16-byte boundary of the address only.
template <int K>
__device__ __forceinline__ void stage_patch_row(float *__restrict__ dst, const float *__restrict__ src, int n, int lane) {
    const int head = min(n, (int)(((16 - (reinterpret_cast<uintptr_t>(src) & 15)) & 15) >> 2));
    const int nvec = (n - head) >> 2;                           // <= 42: one pass of the wave
    if (lane < head) dst[(lane % K) * (kPatchH * kPatchW) + lane / K] = src[lane];
    if (lane < nvec) {
        const float4 x = *reinterpret_cast<const float4 *>(src + head + 4 * lane);
        const float xs[4] = {x.x, x.y, x.z, x.w};
        int e = head + 4 * lane, p = e / K, c = e - p * K;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            dst[c * (kPatchH * kPatchW) + p] = xs[k];
            if (++c == K) { c = 0; ++p; }
        }
    }
    const int e = head + 4 * nvec + lane;                       // tail: at most 3 elements
    if (e < n) dst[(e % K) * (kPatchH * kPatchW) + e / K] = src[e];
}

// the same for a row of u8 storage (K == 3): 16 bytes per vector load, a byte converted by unit_u8 (pixel_dev.h)
__device__ __forceinline__ void stage_patch_row_u8(float *__restrict__ dst, const uint8_t *__restrict__ src, int n, int lane) {
    const int head = min(n, (int)((16 - (reinterpret_cast<uintptr_t>(src) & 15)) & 15));
    const int nvec = (n - head) >> 4;                           // <= 7
    if (lane < head) dst[(lane % 3) * (kPatchH * kPatchW) + lane / 3] = unit_u8(src[lane]);
    if (lane < nvec) {
        const uint4 x = *reinterpret_cast<const uint4 *>(src + head + 16 * lane);
        const uint32_t w[4] = {x.x, x.y, x.z, x.w};
        int e = head + 16 * lane, p = e / 3, c = e - p * 3;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            dst[c * (kPatchH * kPatchW) + p] = unit_u8((uint8_t)(w[k >> 2] >> (8 * (k & 3))));
            if (++c == 3) { c = 0; ++p; }
        }
    }
    const int e = head + 16 * nvec + lane;                      // tail: at most 15 bytes
    if (e < n) dst[(e % 3) * (kPatchH * kPatchW) + e / 3] = unit_u8(src[e]);
}

template <int K>
__global__ void __launch_bounds__(kViewThreads) ssim_views_kernel(
    const float *__restrict__ pred, const float *__restrict__ target, const uint8_t *__restrict__ target_u8, const int64_t *__restrict__ image_ids,
    int64_t pixels_per_image, int H, int W, int tiles_x, int64_t tiles, SsimParams prm, double *__restrict__ partials, double *__restrict__ map) {
    __shared__ float patch[2][K][kPatchH * kPatchW];             // x, y: channel planes of the tile's patch
    __shared__ double planes[kSsimPlanes][kPatchH][kTileW];      // the row-filtered planes of one channel
    const int tid = threadIdx.x, v = blockIdx.y, nb = gridDim.x, b = blockIdx.x;
    const int wave = tid >> 6, lane = tid & 63;
    const int Hc = H - kSsimHalo, Wc = W - kSsimHalo;
    const int lr = tid / kTileW, lc = tid % kTileW;              // this lane's centre of the tile
    const float *xv = pred + (int64_t)v * H * W * K;
    const float *yv = target ? target + (int64_t)v * H * W * K : nullptr;
    const uint8_t *yb = target_u8 ? target_u8 + image_ids[v] * pixels_per_image * 3 : nullptr;
    double *mv = map ? map + (int64_t)v * Hc * Wc : nullptr;
    const int64_t t0 = tiles * b / nb, t1 = tiles * (b + 1) / nb;
    double sum = 0.0;
    for (int64_t t = t0; t < t1; ++t) {
        const int r0 = (int)(t / tiles_x) * kTileH, c0 = (int)(t % tiles_x) * kTileW;
        const int th = min(kTileH, Hc - r0), tw = min(kTileW, Wc - c0);
        const int ph = th + kSsimHalo, pw = tw + kSsimHalo;
        // stage: wave w takes patch rows w, w + 4, ...; the previous tile's last barrier stands between its reads of `patch` and these writes
        for (int pr = wave; pr < ph; pr += kViewThreads / 64) {
            const int64_t off = (int64_t)(r0 + pr) * W + c0;    // first pixel of the patch row
            stage_patch_row<K>(&patch[0][0][pr * kPatchW], xv + off * K, pw * K, lane);
            if (yv) stage_patch_row<K>(&patch[1][0][pr * kPatchW], yv + off * K, pw * K, lane);
            else stage_patch_row_u8(&patch[1][0][pr * kPatchW], yb + off * 3, pw * 3, lane);
        }
        __syncthreads();
        const bool own = lr < th && lc < tw;
        double s_map = 0.0;
#pragma unroll
        for (int ch = 0; ch < K; ++ch) {
            for (int j = tid; j < ph * kTileW; j += kViewThreads) {
                const int pr = j / kTileW, pc = j % kTileW;
                if (pc < tw) {
                    const float *xr = &patch[0][ch][pr * kPatchW + pc], *yr = &patch[1][ch][pr * kPatchW + pc];
                    double a[kSsimPlanes] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
                    for (int k = 0; k < kSsimTaps; ++k) {
                        const double x = (double)xr[k], y = (double)yr[k], g = prm.g[k];
                        a[0] += g * x;
                        a[1] += g * y;
                        a[2] += g * (x * x);
                        a[3] += g * (y * y);
                        a[4] += g * (x * y);
                    }
#pragma unroll
                    for (int p = 0; p < kSsimPlanes; ++p) planes[p][pr][pc] = a[p];
                }
            }
            __syncthreads();
            if (own) {
                double a[kSsimPlanes] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (int k = 0; k < kSsimTaps; ++k) {
                    const double g = prm.g[k];
#pragma unroll
                    for (int p = 0; p < kSsimPlanes; ++p) a[p] += g * planes[p][lr + k][lc];
                }
                const double mx = a[0], my = a[1];
                const double vx = a[2] - mx * mx, vy = a[3] - my * my, cxy = a[4] - mx * my;
                const double num = (2.0 * (mx * my) + prm.c1) * (2.0 * cxy + prm.c2);
                const double den = ((mx * mx + my * my) + prm.c1) * ((vx + vy) + prm.c2);
                const double s = num / den;
                sum += s;
                s_map += s;
            }
            __syncthreads();                                     // the planes are read: the next channel's (or tile's) row pass may overwrite them
        }
        if (own && mv) mv[(int64_t)(r0 + lr) * Wc + (c0 + lc)] = s_map / (double)K;
    }
    const double part[1] = {sum};
    store_partials(part, partials, v, nb, b, tid);
}

// one wave per view
__global__ void __launch_bounds__(64) ssim_finish_kernel(const double *__restrict__ partials, int nb, double count, double *__restrict__ ssim) {
    const int v = blockIdx.x, lane = threadIdx.x;
    double s[1];
    sum_partials(partials, v, nb, lane, s);
    if (lane == 0) ssim[v] = s[0] / count;
}

struct SsimPlan { int tiles_x; ViewPlan vp; };

// H, W >= kSsimTaps
inline SsimPlan ssim_plan(int32_t H, int32_t W) {
    const int tiles_x = (int)ceil_div(W - kSsimHalo, kTileW);
    return {tiles_x, view_plan(ceil_div(H - kSsimHalo, kTileH) * tiles_x, 1)};
}

inline bool ssim_sizes_ok(int32_t n_views, int32_t H, int32_t W, int32_t K) {
    return n_views >= 0 && H >= kSsimTaps && W >= kSsimTaps && K >= 1 && K <= MNF_SSIM_MAX_CHANNELS;
}

template <int K>
void launch_ssim(dim3 grid, hipStream_t s, const float *pred, const float *target, const uint8_t *target_u8, const int64_t *image_ids,
                 int64_t pixels_per_image, int H, int W, const SsimPlan &pl, const SsimParams &prm, double *partials, double *map) {
    hipLaunchKernelGGL(ssim_views_kernel<K>, grid, dim3(kViewThreads), 0, s, pred, target, target_u8, image_ids, pixels_per_image, H, W, pl.tiles_x,
                       pl.vp.tiles, prm, partials, map);
}

}  // namespace
}  // namespace mnf

using namespace mnf;

extern "C" int64_t mnf_ssim_views_workspace_bytes(int32_t n_views, int32_t height, int32_t width, int32_t channels) {
    if (!ssim_sizes_ok(n_views, height, width, channels)) return 0;
    return view_partials_bytes(n_views, ssim_plan(height, width).vp.nb, 1);
}

extern "C" int mnf_ssim_views(const float *pred, const float *target_f32, const uint8_t *target_u8, const int64_t *image_ids,
                              int64_t pixels_per_image, int32_t n_views, int32_t height, int32_t width, int32_t channels, double data_range,
                              double k1, double k2, double *ssim, double *map, void *workspace, int64_t workspace_bytes, mnf_stream_t stream) {
    MNF_REQUIRE(n_views >= 0, "ssim_views: n_views is negative (%d)", n_views);
    MNF_REQUIRE(height >= kSsimTaps && width >= kSsimTaps, "ssim_views: the 11 x 11 window needs height and width >= 11 (got %d x %d)", height, width);
    MNF_REQUIRE(channels >= 1 && channels <= MNF_SSIM_MAX_CHANNELS, "ssim_views: channels must be 1 .. %d (got %d)", MNF_SSIM_MAX_CHANNELS, channels);
    MNF_REQUIRE(finite_d(data_range) && data_range > 0.0, "ssim_views: data_range must be finite and positive (got %g)", data_range);
    MNF_REQUIRE(finite_d(k1) && k1 >= 0.0 && finite_d(k2) && k2 >= 0.0, "ssim_views: k1 and k2 must be finite and not negative (got %g, %g)", k1, k2);
    MNF_REQUIRE(n_views <= 65535, "ssim_views: at most 65535 views per call (got %d)", n_views);
    if (n_views == 0) return MNF_OK;
    MNF_REQUIRE((target_f32 != nullptr) != (target_u8 != nullptr), "ssim_views: exactly one of target_f32 and target_u8 must be given");
    if (target_u8) {
        MNF_REQUIRE(channels == 3, "ssim_views: the u8 target is rgb storage and needs channels == 3 (got %d)", channels);
        MNF_REQUIRE(pixels_per_image == (int64_t)height * width, "ssim_views: the u8 target holds whole images: pixels_per_image (%lld) must be height * width (%lld)",
                    (long long)pixels_per_image, (long long)height * width);
    }
    MNF_REQUIRE(pred, "ssim_views: pred is null");
    MNF_REQUIRE(!target_u8 || image_ids, "ssim_views: the u8 target needs image_ids");
    MNF_REQUIRE(aligned4(pred) && aligned4(target_f32), "ssim_views: the fp32 planes must be 4-byte aligned");
    MNF_REQUIRE(ssim, "ssim_views: ssim is null");
    MNF_REQUIRE(aligned8(ssim), "ssim_views: ssim must be 8-byte aligned");
    MNF_REQUIRE(aligned8(map), "ssim_views: map must be 8-byte aligned");
    const SsimPlan pl = ssim_plan(height, width);
    const int64_t need = view_partials_bytes(n_views, pl.vp.nb, 1);
    MNF_REQUIRE(workspace && aligned8(workspace), "ssim_views: needs an 8-byte aligned workspace");
    MNF_REQUIRE(workspace_bytes >= need, "ssim_views: workspace too small (%lld < %lld bytes)", (long long)workspace_bytes, (long long)need);
    SsimParams prm;
    double gsum = 0.0;
    for (int i = 0; i < kSsimTaps; ++i) {
        const double d = (double)(i - kSsimTaps / 2) / MNF_SSIM_SIGMA;
        prm.g[i] = std::exp(-0.5 * (d * d));
        gsum += prm.g[i];
    }
    for (int i = 0; i < kSsimTaps; ++i) prm.g[i] /= gsum;
    prm.c1 = (k1 * data_range) * (k1 * data_range);
    prm.c2 = (k2 * data_range) * (k2 * data_range);
    hipStream_t s = as_stream(stream);
    ProfScope prof("ssim_views", s);
    double *partials = reinterpret_cast<double *>(workspace);
    const dim3 grid(pl.vp.nb, n_views);
    switch (channels) {
    case 1: launch_ssim<1>(grid, s, pred, target_f32, target_u8, image_ids, pixels_per_image, height, width, pl, prm, partials, map); break;
    case 2: launch_ssim<2>(grid, s, pred, target_f32, target_u8, image_ids, pixels_per_image, height, width, pl, prm, partials, map); break;
    case 3: launch_ssim<3>(grid, s, pred, target_f32, target_u8, image_ids, pixels_per_image, height, width, pl, prm, partials, map); break;
    default: launch_ssim<4>(grid, s, pred, target_f32, target_u8, image_ids, pixels_per_image, height, width, pl, prm, partials, map); break;
    }
    int rc = launch_status("ssim_views_kernel");
    if (rc) return rc;
    const double count = (double)((int64_t)(height - kSsimHalo) * (width - kSsimHalo) * channels);
    hipLaunchKernelGGL(ssim_finish_kernel, dim3(n_views), dim3(64), 0, s, partials, pl.vp.nb, count, ssim);
    return launch_status("ssim_finish_kernel");
}
