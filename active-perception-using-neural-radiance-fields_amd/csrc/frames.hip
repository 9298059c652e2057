// 8-bit frames of finished renders on the device (gfx950):
//   mnf_frames_views  <- scripts/pipeline.py:976-1023 (per pose of the chosen trajectory: np.float32(rgb * 255), np.clip(dep * 25, 0, 255),
//                        acc * 255, np.argmax over the float64 [h, w, C] stack, the colour palette indexed by the label, cv2.cvtColor to
//                        BGR, and cv2.imwrite narrowing each plane to 8 bits) and visualization/vis_nerf_habitat.py:142-179 (the same per
//                        viewer pose with clip(depth / 10, 0, 1) * 255)
//
// One streaming pass over the finished planes of V views of P pixels: (3 + 1 + 1 + C) * 4 bytes are read per pixel, once, and
// 3 + 1 + 1 + 3 (+ 1 with the label plane) bytes are written.
//
// The work split and the logit staging are view_dev.h's; the stage exists only when a label is needed (a tile is 256 pixels otherwise).
//
// Every byte is a chain of separately rounded operations (this file is compiled with -ffp-contract=off):
//   sat8(x)  = view_dev.h's: x clamped to [0, 255] and rounded to nearest, ties to even; NaN -> 0, +inf -> 255, -inf -> 0
//   rgb8     = sat8(x * 255.0f), the product rounded to float32: np.float32(float64(x) * 255) is that number, since x * 255 is exact in
//              float64 and is then rounded once
//   occ8     = sat8((double)acc * 255.0)
//   dep8     = sat8(clip(((double)d * depth_mul) / depth_div, 0, depth_clip_hi) * depth_gain) in float64, numpy's arithmetic on the float64
//              stacks; clip = np.clip = minimum(maximum(x, 0), hi), a NaN stays a NaN
//   labels   = first maximal logit, a NaN counts as the maximum (np.argmax);  sem8 = palette[label]
//
// The outputs may start at any byte (a view's 3 * P-byte plane is not dword-aligned when P is odd), so a lane does not store its own
// bytes: a tile's bytes of each plane are assembled in LDS, shifted by the destination's offset inside its dword, and go out as whole
// aligned dwords, one per lane; the (at most two) dwords that the tile only partly owns are stored byte by byte.  Nothing outside
// an output's [V * P * k] bytes is written, and nothing inside it is read.
#include "view_dev.h"

namespace mnf {
namespace {

constexpr int kFramesWords3 = (kViewThreads * 3 + 3) / 4 + 1;      // dwords of a tile's 3-byte plane shifted by up to 3 bytes
constexpr int kFramesWords1 = (kViewThreads + 3) / 4 + 1;

struct FrameDepth { double mul, div, hi, gain; };

// Store the n bytes buf[mis .. mis + n) to dst[0 .. n), mis = dst & 3: dword w of `buf` is the aligned global dword at dst - mis + 4 w.
__device__ __forceinline__ void flush_plane(const uint32_t *buf, uint8_t *__restrict__ dst, int n, int tid) {
    const int mis = byte_in_word(dst);
    const int end = mis + n, nw = (end + 3) >> 2;
    uint8_t *base = dst - mis;
    const uint8_t *bytes = reinterpret_cast<const uint8_t *>(buf);
    for (int w = tid; w < nw; w += kViewThreads) {
        const int lo = 4 * w, hi = lo + 4;
        if (lo >= mis && hi <= end) {
            *reinterpret_cast<uint32_t *>(base + lo) = buf[w];
        } else {
            const int b0 = lo > mis ? lo : mis, b1 = hi < end ? hi : end;
            for (int b = b0; b < b1; ++b) base[b] = bytes[b];
        }
    }
}

__global__ void __launch_bounds__(kViewThreads) frames_views_kernel(
    const float *__restrict__ rgb, const float *__restrict__ depth, const float *__restrict__ acc, const float *__restrict__ sem, int64_t P, int C,
    int tp, int64_t tiles, const uint8_t *__restrict__ palette, FrameDepth dm, int bgr, uint8_t *__restrict__ rgb8,
    uint8_t *__restrict__ dep8, uint8_t *__restrict__ occ8, uint8_t *__restrict__ sem8, uint8_t *__restrict__ labels) {
    extern __shared__ float stage[];                               // [tp][C | 1], only when a label is needed
    __shared__ uint32_t out3[2][kFramesWords3];                    // rgb8, sem8
    __shared__ uint32_t out1[3][kFramesWords1];                    // dep8, occ8, labels
    const int tid = threadIdx.x, v = blockIdx.y, nb = gridDim.x, b = blockIdx.x;
    const int Cs = C | 1;
    const bool want_label = sem8 || labels;
    const int c0 = bgr ? 2 : 0, c2 = 2 - c0;
    const int64_t t0 = tiles * b / nb, t1 = tiles * (b + 1) / nb;
    for (int64_t t = t0; t < t1; ++t) {
        const int64_t p0 = t * tp, i0 = (int64_t)v * P + p0;
        const int np = (int)(P - p0 < tp ? P - p0 : tp);
        __syncthreads();                                           // the previous tile's rows are read and its bytes are out
        if (want_label) {
            stage_rows(stage, sem + i0 * C, np * C, C, Cs, tid);
            __syncthreads();
        }
        uint8_t *d_rgb = rgb8 ? rgb8 + 3 * i0 : nullptr, *d_sem = sem8 ? sem8 + 3 * i0 : nullptr;
        uint8_t *d_dep = dep8 ? dep8 + i0 : nullptr, *d_occ = occ8 ? occ8 + i0 : nullptr, *d_lab = labels ? labels + i0 : nullptr;
        if (tid < np) {
            const int64_t i = i0 + tid;
            if (rgb8) {
                uint8_t *o = reinterpret_cast<uint8_t *>(out3[0]) + byte_in_word(d_rgb) + 3 * tid;
                o[c0] = sat8(rgb[3 * i] * 255.0f);
                o[1] = sat8(rgb[3 * i + 1] * 255.0f);
                o[c2] = sat8(rgb[3 * i + 2] * 255.0f);
            }
            if (dep8) {
                const double x = ((double)depth[i] * dm.mul) / dm.div;
                const double lo = x < 0.0 ? 0.0 : x;               // np.maximum(x, 0): a NaN fails the comparison and stays
                const double cl = lo > dm.hi ? dm.hi : lo;         // np.minimum(., hi)
                reinterpret_cast<uint8_t *>(out1[0])[byte_in_word(d_dep) + tid] = sat8(cl * dm.gain);
            }
            if (occ8) reinterpret_cast<uint8_t *>(out1[1])[byte_in_word(d_occ) + tid] = sat8((double)acc[i] * 255.0);
            if (want_label) {
                float best;
                const int arg = first_argmax(stage + tid * Cs, C, &best);
                if (labels) reinterpret_cast<uint8_t *>(out1[2])[byte_in_word(d_lab) + tid] = (uint8_t)arg;
                if (sem8) {
                    uint8_t *o = reinterpret_cast<uint8_t *>(out3[1]) + byte_in_word(d_sem) + 3 * tid;
                    o[c0] = palette[3 * arg];
                    o[1] = palette[3 * arg + 1];
                    o[c2] = palette[3 * arg + 2];
                }
            }
        }
        __syncthreads();
        if (rgb8) flush_plane(out3[0], d_rgb, 3 * np, tid);
        if (sem8) flush_plane(out3[1], d_sem, 3 * np, tid);
        if (dep8) flush_plane(out1[0], d_dep, np, tid);
        if (occ8) flush_plane(out1[1], d_occ, np, tid);
        if (labels) flush_plane(out1[2], d_lab, np, tid);
    }
}

}  // namespace
}  // namespace mnf

using namespace mnf;

extern "C" int mnf_frames_views(const float *rgb, const float *depth, const float *acc, const float *sem, int32_t n_views, int64_t n_pix,
                                int32_t n_classes, const uint8_t *palette, int32_t palette_entries, double depth_mul, double depth_div,
                                double depth_clip_hi, double depth_gain, int32_t bgr, uint8_t *rgb8, uint8_t *dep8, uint8_t *occ8, uint8_t *sem8,
                                uint8_t *labels, mnf_stream_t stream) {
    MNF_REQUIRE(n_views >= 0, "frames_views: n_views is negative (%d)", n_views);
    MNF_REQUIRE(n_pix > 0, "frames_views: n_pix must be positive (got %lld)", (long long)n_pix);
    MNF_REQUIRE(n_classes > 0, "frames_views: n_classes must be positive (got %d)", n_classes);
    MNF_REQUIRE(palette_entries >= 0, "frames_views: palette_entries is negative (%d)", palette_entries);
    MNF_REQUIRE(!labels || n_classes <= 256, "frames_views: labels holds uint8 class ids and needs n_classes <= 256 (got %d)", n_classes);
    MNF_REQUIRE(finite_d(depth_mul) && finite_d(depth_div) && finite_d(depth_clip_hi) && finite_d(depth_gain),
                "frames_views: depth_mul, depth_div, depth_clip_hi and depth_gain must be finite (got %g, %g, %g, %g)", depth_mul, depth_div,
                depth_clip_hi, depth_gain);
    MNF_REQUIRE(depth_div != 0.0, "frames_views: depth_div is zero");
    const bool want_label = sem8 || labels;
    MNF_REQUIRE(!want_label || palette_entries >= n_classes, "frames_views: palette_entries (%d) is less than n_classes (%d)", palette_entries, n_classes);
    if (n_views == 0) return MNF_OK;
    MNF_REQUIRE(!rgb8 || rgb, "frames_views: rgb is null");
    MNF_REQUIRE(!dep8 || depth, "frames_views: depth is null");
    MNF_REQUIRE(!occ8 || acc, "frames_views: acc is null");
    MNF_REQUIRE(!want_label || sem, "frames_views: sem is null");
    MNF_REQUIRE(!want_label || palette, "frames_views: palette is null");
    MNF_REQUIRE(n_views <= 65535, "frames_views: at most 65535 views per call (got %d)", n_views);
    int tp = kViewThreads;
    if (want_label) {
        tp = stage_tile_pixels(n_classes);
        if (tp < 1) {
            set_error("frames_views: n_classes = %d is more than one LDS tile holds (%d)", n_classes, kStageBytes / 4 - 1);
            return MNF_ERR_UNSUPPORTED;
        }
    }
    if (!rgb8 && !dep8 && !occ8 && !want_label) return MNF_OK;     // every output skipped
    const ViewPlan pl = view_plan(n_pix, tp);
    hipStream_t s = as_stream(stream);
    ProfScope prof("frames_views", s);
    const size_t lds = want_label ? (size_t)tp * (n_classes | 1) * sizeof(float) : 0;
    const FrameDepth dm = {depth_mul, depth_div, depth_clip_hi, depth_gain};
    hipLaunchKernelGGL(frames_views_kernel, dim3(pl.nb, n_views), dim3(kViewThreads), lds, s, rgb, depth, acc, sem, n_pix, n_classes, tp, pl.tiles,
                       palette, dm, bgr != 0, rgb8, dep8, occ8, sem8, labels);
    return launch_status("frames_views_kernel");
}
