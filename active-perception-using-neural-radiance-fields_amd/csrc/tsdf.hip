// TSDF fusion of captures on the device (gfx950): the truncated signed distance volume a classical robotics stack builds from the depth,
// colour and class images the field is trained on, its lattice for the observed-only surface extractor and the attributes of mesh vertices.
//   mnf_tsdf_integrate     V views folded into the volume, in ascending view order, one launch
//   mnf_tsdf_lattice       -tsdf where observed, NaN elsewhere, and three counts
//   mnf_tsdf_vertex_attrs  colour and class of a vertex from the best-observed corner of its cell
// include/mi355nerf.h ("TSDF fusion of captures") has the definition; every output byte of this unit is fixed by it.  Built with
// -ffp-contract=off: a point's projection and its update are chains of separately rounded float64 operations, as numpy evaluates them
// (tests/tsdf_ref.py).
//
// integrate_kernel.  One lane per lattice point; a workgroup of 256 lanes owns a block of kBX x kBY x kBZ points, z fastest within the
// block as in memory, so a wave's loads and stores of the four state arrays are runs of kBZ * 4 bytes.  A lane's state lives in registers
// over the whole view loop: loaded once before the first view that survives the cull, stored once, and only by a wave one of whose lanes
// a view changed.  The views are taken 256 at a time: lane t tests view base + t against the block's bounding sphere (the near plane and
// the four frustum planes, in camera coordinates, with the columns' norms in the bound so that a pose need not be orthonormal, and a slack
// far above the rounding of the per-point chain), a ballot per wave compacts the survivors into LDS in ascending order, and the workgroup
// loops over that list with a uniform trip count.  The view index is made wave-uniform with readfirstlane, so the 12 doubles of its pose
// are scalar loads.  Depth, colour and class are gathers: neighbouring points fall on neighbouring pixels, and the caches serve them.
// There is no cull on max_depth: the header counts far points as behind the surface or as invalid depths.  The five counters are summed
// per wave (shuffles), per workgroup (LDS) and added with one integer atomic each: integer sums, the same whatever the schedule.  No
// atomic touches the state.
//
// The block shape is a compile-time choice (MNF_TSDF_BLOCK: 0 = 4 x 4 x 16, 1 = 1 x 4 x 64, 2 = 2 x 8 x 16); tools/tsdf_measure.py and
// DESIGN.md say which were measured and which stayed.
#include "reduce_dev.h"
#include "workspace.h"

#ifndef MNF_TSDF_BLOCK
#define MNF_TSDF_BLOCK 0
#endif

namespace mnf {
namespace {

constexpr int kThreads = 256;
constexpr int kMaxCells = 1024;                      // per axis, as mnf_surface_extract
constexpr int kMaxViews = MNF_TSDF_MAX_VIEWS;
#if MNF_TSDF_BLOCK == 1
constexpr int kBX = 1, kBY = 4, kBZ = 64;
#elif MNF_TSDF_BLOCK == 2
constexpr int kBX = 2, kBY = 8, kBZ = 16;
#else
constexpr int kBX = 4, kBY = 4, kBZ = 16;
#endif
static_assert(kBX * kBY * kBZ == kThreads, "a block of points is one workgroup");

struct Volume {
    int NX, NY, NZ;                                   // points per axis
    int bx, by, bz;                                   // blocks per axis
    double lo[3], voxel, trunc;
    int max_weight;
    double min_depth, max_depth;
};

struct Camera {
    int W, H;
    double focal;
    int depth_f16, stride, class_i64, ray;
};

__device__ __forceinline__ double load_depth(const void *depth, int f16, int64_t p) {
    return f16 ? (double)(float)reinterpret_cast<const _Float16 *>(depth)[p] : (double)reinterpret_cast<const float *>(depth)[p];
}

// true when no point within `r` of the block's centre can pass steps 3 and 4 of the header for view m
__device__ __forceinline__ bool view_misses(const double *__restrict__ m, const double ctr[3], double r, const Volume &vol, const Camera &cam) {
    const double q0 = ctr[0] - m[3], q1 = ctr[1] - m[7], q2 = ctr[2] - m[11];
    const double xc = (q0 * m[0] + q1 * m[4]) + q2 * m[8], yc = (q0 * m[1] + q1 * m[5]) + q2 * m[9], zc = (q0 * m[2] + q1 * m[6]) + q2 * m[10];
    const double n0 = sqrt((m[0] * m[0] + m[4] * m[4]) + m[8] * m[8]), n1 = sqrt((m[1] * m[1] + m[5] * m[5]) + m[9] * m[9]),
                 n2 = sqrt((m[2] * m[2] + m[6] * m[6]) + m[10] * m[10]);
    // the centre and the camera are rounded too: widen the sphere by far more than that
    const double re = r * 1.000001 + 1e-9 * (((fabs(ctr[0]) + fabs(ctr[1])) + fabs(ctr[2])) + ((fabs(m[3]) + fabs(m[7])) + fabs(m[11])));
    const double zd = -zc, hw = 0.5 * (double)cam.W, hh = 0.5 * (double)cam.H, f = cam.focal;
    // near plane: every point has zd <= zd_c + re n2
    if (zd + re * n2 < vol.min_depth - 1e-9 * (fabs(zd) + fabs(vol.min_depth))) return true;
    // the four planes, for zd > 0: 0 <= u < W  <=>  xc f + zd W/2 >= 0 and xc f - zd W/2 < 0; the same for -yc and H
    const double bx = re * (f * n0 + hw * n2), by = re * (f * n1 + hh * n2);
    const double tx = f * fabs(xc) + hw * fabs(zd), ty = f * fabs(yc) + hh * fabs(zd);
    const double sx = 1e-9 * (tx + bx), sy = 1e-9 * (ty + by);
    if ((xc * f - zd * hw) - bx > sx) return true;
    if (-(xc * f + zd * hw) - bx > sx) return true;
    if (((-yc) * f - zd * hh) - by > sy) return true;
    if (-((-yc) * f + zd * hh) - by > sy) return true;
    return false;                                     // a NaN anywhere fails every test above: the view is kept
}

__global__ void __launch_bounds__(kThreads) integrate_kernel(float *__restrict__ tsdf, int32_t *__restrict__ weight, uint32_t *__restrict__ word,
                                                             float *__restrict__ best, Volume vol, Camera cam, const double *__restrict__ c2w, int n_views,
                                                             const void *__restrict__ depth, const uint8_t *__restrict__ colour,
                                                             const void *__restrict__ classes, unsigned long long *__restrict__ info) {
    __shared__ int s_list[kThreads];
    __shared__ int s_wave_n[kThreads / 64];
    __shared__ int s_counts[kThreads / 64][5];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    int b = blockIdx.x;
    const int bz = b % vol.bz;
    b /= vol.bz;
    const int by = b % vol.by, bx = b / vol.by;
    const int x0 = bx * kBX, y0 = by * kBY, z0 = bz * kBZ;
    const int x = x0 + t / (kBY * kBZ), y = y0 + (t / kBZ) % kBY, z = z0 + t % kBZ;
    const bool live = x < vol.NX && y < vol.NY && z < vol.NZ;
    const int64_t lin = ((int64_t)x * vol.NY + y) * vol.NZ + z;
    const double w0 = vol.lo[0] + (double)x * vol.voxel, w1 = vol.lo[1] + (double)y * vol.voxel, w2 = vol.lo[2] + (double)z * vol.voxel;

    // the block's bounding sphere, over the points that exist
    const int x1 = (x0 + kBX < vol.NX ? x0 + kBX : vol.NX) - 1, y1 = (y0 + kBY < vol.NY ? y0 + kBY : vol.NY) - 1, z1 = (z0 + kBZ < vol.NZ ? z0 + kBZ : vol.NZ) - 1;
    const double ctr[3] = {vol.lo[0] + 0.5 * (double)(x0 + x1) * vol.voxel, vol.lo[1] + 0.5 * (double)(y0 + y1) * vol.voxel,
                           vol.lo[2] + 0.5 * (double)(z0 + z1) * vol.voxel};
    const double ex = (double)(x1 - x0), ey = (double)(y1 - y0), ez = (double)(z1 - z0);
    const double radius = 0.5 * vol.voxel * sqrt((ex * ex + ey * ey) + ez * ez);

    float r_tsdf = 1.0f, r_best = -1.0f;
    int r_weight = 0;
    uint32_t r_word = 0;
    bool loaded = false, dirty = false;
    int c_applied = 0, c_first = 0, c_invalid = 0, c_behind = 0, c_label = 0;

    for (int base = 0; base < n_views; base += kThreads) {
        const int mine = base + t;
        const bool keep = mine < n_views && !view_misses(c2w + (int64_t)mine * 12, ctr, radius, vol, cam);
        const unsigned long long ballot = __ballot(keep);
        __syncthreads();                                                          // the previous chunk's list is no longer read
        if (lane == 0) s_wave_n[wave] = __popcll(ballot);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int k = 0; k < kThreads / 64; ++k) {
            const int n = s_wave_n[k];
            before += k < wave ? n : 0;
            total += n;
        }
        if (keep) s_list[before + __popcll(ballot & ((1ull << lane) - 1ull))] = mine;
        __syncthreads();
        if (total == 0) continue;                                                 // (uniform)
        if (!loaded) {
            loaded = true;
            if (live) { r_tsdf = tsdf[lin]; r_weight = weight[lin]; r_word = word[lin]; r_best = best[lin]; }
        }
        for (int i = 0; i < total; ++i) {
            const int v = __builtin_amdgcn_readfirstlane(s_list[i]);
            const double *__restrict__ m = c2w + (int64_t)v * 12;
            if (!live) continue;
            const double q0 = w0 - m[3], q1 = w1 - m[7], q2 = w2 - m[11];
            const double xc = (q0 * m[0] + q1 * m[4]) + q2 * m[8], yc = (q0 * m[1] + q1 * m[5]) + q2 * m[9], zc = (q0 * m[2] + q1 * m[6]) + q2 * m[10];
            const double zd = -zc;
            if (!(zd > vol.min_depth)) continue;
            const double u = floor((xc / zd) * cam.focal + (double)cam.W * 0.5), vv = floor(((-yc) / zd) * cam.focal + (double)cam.H * 0.5);
            if (!(u >= 0.0 && u < (double)cam.W && vv >= 0.0 && vv < (double)cam.H)) continue;
            const int64_t p = ((int64_t)v * cam.H + (int)vv) * cam.W + (int)u;
            const double d = load_depth(depth, cam.depth_f16, p);
            if (!(finite_d(d) && d > 0.0 && d <= vol.max_depth)) { ++c_invalid; continue; }
            const double along = cam.ray ? sqrt((q0 * q0 + q1 * q1) + q2 * q2) : zd;
            const double sdf = d - along;
            if (sdf < -vol.trunc) { ++c_behind; continue; }
            const double ratio = sdf / vol.trunc;
            const double s = ratio < 1.0 ? ratio : 1.0;
            r_tsdf = (float)(((double)r_tsdf * (double)r_weight + s) / (double)(r_weight + 1));
            ++c_applied;
            c_first += r_weight == 0 ? 1 : 0;
            r_weight = r_weight + 1 < vol.max_weight ? r_weight + 1 : vol.max_weight;
            dirty = true;
            const double a = fabs(sdf);
            if (a <= vol.trunc && (r_best < 0.0f || (float)a < r_best)) {
                r_best = (float)a;
                const uint8_t *c = colour + p * cam.stride;
                uint32_t cls;
                if (cam.class_i64) {
                    const int64_t k = reinterpret_cast<const int64_t *>(classes)[p];
                    if (k < 0 || k > 255) { cls = 255u; ++c_label; } else cls = (uint32_t)k;
                } else {
                    cls = reinterpret_cast<const uint8_t *>(classes)[p];
                }
                r_word = (uint32_t)c[0] | ((uint32_t)c[1] << 8) | ((uint32_t)c[2] << 16) | (cls << 24);
            }
        }
    }
    if (!loaded) return;                                                          // (uniform) no view reaches this block: nothing read, nothing written
    if (__ballot(dirty) && live) { tsdf[lin] = r_tsdf; weight[lin] = r_weight; word[lin] = r_word; best[lin] = r_best; }
    wave_sum_each(c_applied, c_first, c_invalid, c_behind, c_label);
    if (lane == 0) {
        s_counts[wave][0] = c_applied; s_counts[wave][1] = c_first; s_counts[wave][2] = c_invalid; s_counts[wave][3] = c_behind; s_counts[wave][4] = c_label;
    }
    __syncthreads();
    if (t < 5) {
        int n = 0;
#pragma unroll
        for (int k = 0; k < kThreads / 64; ++k) n += s_counts[k][t];
        if (n) atomicAdd(info + t, (unsigned long long)n);
    }
}

__global__ void __launch_bounds__(kThreads) lattice_kernel(const float *__restrict__ tsdf, const int32_t *__restrict__ weight, const float *__restrict__ best,
                                                           int64_t n, int min_weight, float *__restrict__ values, unsigned long long *__restrict__ counts) {
    __shared__ int s_counts[kThreads / 64][3];
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    int c_obs = 0, c_in = 0, c_word = 0;
    if (i < n) {
        const bool obs = weight[i] >= min_weight;
        const float v = tsdf[i];
        values[i] = obs ? -v : __int_as_float(0x7fc00000);
        c_obs = obs ? 1 : 0;
        c_in = obs && v < 0.0f ? 1 : 0;
        c_word = best[i] >= 0.0f ? 1 : 0;
    }
    wave_sum_each(c_obs, c_in, c_word);
    if ((threadIdx.x & 63) == 0) { s_counts[threadIdx.x >> 6][0] = c_obs; s_counts[threadIdx.x >> 6][1] = c_in; s_counts[threadIdx.x >> 6][2] = c_word; }
    __syncthreads();
    if (threadIdx.x < 3) {
        int s = 0;
#pragma unroll
        for (int k = 0; k < kThreads / 64; ++k) s += s_counts[k][threadIdx.x];
        if (s) atomicAdd(counts + threadIdx.x, (unsigned long long)s);
    }
}

struct Cells { int X, Y, Z; double lo[3], voxel; };

__global__ void __launch_bounds__(kThreads) attrs_kernel(const uint32_t *__restrict__ word, const float *__restrict__ best, Cells g,
                                                         const float *__restrict__ positions, int64_t n, const uint8_t *__restrict__ palette, int n_palette,
                                                         uint8_t *__restrict__ colour, int32_t *__restrict__ label, uint8_t *__restrict__ sem_colour) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const int N[3] = {g.X, g.Y, g.Z};
    int c[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double p = floor(((double)positions[3 * i + k] - g.lo[k]) / g.voxel);
        c[k] = !(p >= 0.0) ? 0 : p > (double)(N[k] - 1) ? N[k] - 1 : (int)p;
    }
    const int sy = g.Z + 1, sx = (g.Y + 1) * sy;
    const int64_t lin0 = ((int64_t)c[0] * (g.Y + 1) + c[1]) * (g.Z + 1) + c[2];
    float b_best = -1.0f;
    uint32_t b_word = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {                                                // ascending lin: x slowest
        const int64_t q = lin0 + ((k >> 2) & 1) * sx + ((k >> 1) & 1) * sy + (k & 1);
        const float b = best[q];
        if (b >= 0.0f && (b_best < 0.0f || b < b_best)) { b_best = b; b_word = word[q]; }
    }
    const bool got = b_best >= 0.0f;
    const int lab = got ? (int)(b_word >> 24) : -1;
    if (colour) {
#pragma unroll
        for (int k = 0; k < 3; ++k) colour[3 * i + k] = got ? (uint8_t)(b_word >> (8 * k)) : (uint8_t)0;
    }
    if (label) label[i] = lab;
    if (sem_colour) {
        const bool ok = lab >= 0 && lab < n_palette;
#pragma unroll
        for (int k = 0; k < 3; ++k) sem_colour[3 * i + k] = ok ? palette[3 * lab + k] : (uint8_t)0;
    }
}

inline bool cells_ok(int32_t X, int32_t Y, int32_t Z) { return X >= 1 && Y >= 1 && Z >= 1 && X <= kMaxCells && Y <= kMaxCells && Z <= kMaxCells; }
inline bool positive_d(double v) { return v > 0.0 && finite_d(v); }

}  // namespace
}  // namespace mnf

using namespace mnf;

extern "C" int mnf_tsdf_integrate(float *tsdf, int32_t *weight, uint32_t *word, float *best, int32_t cells_x, int32_t cells_y, int32_t cells_z,
                                  const double *lo_host, double voxel, double trunc, int32_t max_weight, double min_depth, double max_depth, const double *c2w,
                                  int32_t n_views, int32_t width, int32_t height, double focal, const void *depth, int32_t depth_type, const uint8_t *colour,
                                  int32_t colour_stride, const void *classes, int32_t class_type, int32_t depth_mode, int64_t *info, mnf_stream_t stream) {
    MNF_REQUIRE(cells_ok(cells_x, cells_y, cells_z), "tsdf_integrate: cells per axis must lie in 1 .. %d (got %d x %d x %d)", kMaxCells, cells_x, cells_y, cells_z);
    MNF_REQUIRE(lo_host, "tsdf_integrate: lo_host is null");
    for (int k = 0; k < 3; ++k) MNF_REQUIRE(finite_d(lo_host[k]), "tsdf_integrate: lo_host[%d] is not finite", k);
    MNF_REQUIRE(positive_d(voxel), "tsdf_integrate: voxel must be positive and finite (got %g)", voxel);
    MNF_REQUIRE(positive_d(trunc), "tsdf_integrate: trunc must be positive and finite (got %g)", trunc);
    MNF_REQUIRE(max_weight >= 1, "tsdf_integrate: max_weight outside 1 .. 2^31 - 1 (got %d)", max_weight);
    MNF_REQUIRE(min_depth >= 0.0 && finite_d(min_depth), "tsdf_integrate: min_depth must be finite and not negative (got %g)", min_depth);
    MNF_REQUIRE(max_depth > min_depth && finite_d(max_depth), "tsdf_integrate: max_depth must be finite and above min_depth (got %g)", max_depth);
    MNF_REQUIRE(n_views >= 0 && n_views <= kMaxViews, "tsdf_integrate: n_views outside 0 .. %d (got %d)", kMaxViews, n_views);
    MNF_REQUIRE(width > 0 && height > 0 && width <= 16384 && height <= 16384, "tsdf_integrate: the image is %d x %d (1 .. 16384 each)", width, height);
    MNF_REQUIRE(positive_d(focal), "tsdf_integrate: focal must be positive and finite (got %g)", focal);
    MNF_REQUIRE(depth_type == MNF_TSDF_DEPTH_F32 || depth_type == MNF_TSDF_DEPTH_F16, "tsdf_integrate: depth_type %d is neither f32 nor f16", depth_type);
    MNF_REQUIRE(colour_stride == 3 || colour_stride == 4, "tsdf_integrate: colour_stride is 3 or 4 (got %d)", colour_stride);
    MNF_REQUIRE(class_type == MNF_TSDF_CLASS_U8 || class_type == MNF_TSDF_CLASS_I64, "tsdf_integrate: class_type %d is neither uint8 nor int64", class_type);
    MNF_REQUIRE(depth_mode == MNF_SENSOR_DEPTH_PLANAR || depth_mode == MNF_SENSOR_DEPTH_RAY, "tsdf_integrate: depth_mode %d is neither planar nor ray", depth_mode);
    MNF_REQUIRE(tsdf && weight && word && best, "tsdf_integrate: a null state array");
    MNF_REQUIRE(aligned4(tsdf) && aligned4(weight) && aligned4(word) && aligned4(best), "tsdf_integrate: the state arrays must be 4-byte aligned");
    MNF_REQUIRE(info, "tsdf_integrate: info is null");
    MNF_REQUIRE(aligned8(info), "tsdf_integrate: info must be 8-byte aligned");
    MNF_REQUIRE((c2w && depth && colour && classes) || n_views == 0, "tsdf_integrate: a null pose or image array");
    MNF_REQUIRE(aligned8(c2w), "tsdf_integrate: c2w must be 8-byte aligned");
    MNF_REQUIRE(depth_type == MNF_TSDF_DEPTH_F32 ? aligned4(depth) : (reinterpret_cast<uintptr_t>(depth) & 1) == 0, "tsdf_integrate: depth is misaligned");
    MNF_REQUIRE(class_type == MNF_TSDF_CLASS_U8 || aligned8(classes), "tsdf_integrate: int64 classes must be 8-byte aligned");
    if (n_views == 0) return MNF_OK;
    Volume vol;
    vol.NX = cells_x + 1; vol.NY = cells_y + 1; vol.NZ = cells_z + 1;
    vol.bx = (vol.NX + kBX - 1) / kBX; vol.by = (vol.NY + kBY - 1) / kBY; vol.bz = (vol.NZ + kBZ - 1) / kBZ;
    for (int k = 0; k < 3; ++k) vol.lo[k] = lo_host[k];
    vol.voxel = voxel; vol.trunc = trunc; vol.max_weight = max_weight; vol.min_depth = min_depth; vol.max_depth = max_depth;
    const Camera cam = {width, height, focal, depth_type == MNF_TSDF_DEPTH_F16, colour_stride, class_type == MNF_TSDF_CLASS_I64, depth_mode == MNF_SENSOR_DEPTH_RAY};
    const int64_t blocks = (int64_t)vol.bx * vol.by * vol.bz;                     // <= 1025 * 257 * 65: far below 2^31
    hipStream_t s = as_stream(stream);
    ProfScope prof("tsdf_integrate", s);
    hipLaunchKernelGGL(integrate_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, s, tsdf, weight, word, best, vol, cam, c2w, n_views, depth, colour, classes,
                       reinterpret_cast<unsigned long long *>(info));
    return launch_status("integrate_kernel");
}

extern "C" int mnf_tsdf_lattice(const float *tsdf, const int32_t *weight, const float *best, int32_t cells_x, int32_t cells_y, int32_t cells_z,
                                int32_t min_weight, float *values, int64_t *counts, mnf_stream_t stream) {
    MNF_REQUIRE(cells_ok(cells_x, cells_y, cells_z), "tsdf_lattice: cells per axis must lie in 1 .. %d (got %d x %d x %d)", kMaxCells, cells_x, cells_y, cells_z);
    MNF_REQUIRE(min_weight >= 1, "tsdf_lattice: min_weight outside 1 .. 2^31 - 1 (got %d)", min_weight);
    MNF_REQUIRE(tsdf && weight && best, "tsdf_lattice: a null state array");
    MNF_REQUIRE(aligned4(tsdf) && aligned4(weight) && aligned4(best), "tsdf_lattice: the state arrays must be 4-byte aligned");
    MNF_REQUIRE(values, "tsdf_lattice: values is null");
    MNF_REQUIRE(aligned4(values), "tsdf_lattice: values must be 4-byte aligned");
    MNF_REQUIRE(counts, "tsdf_lattice: counts is null");
    MNF_REQUIRE(aligned8(counts), "tsdf_lattice: counts must be 8-byte aligned");
    const int64_t n = (int64_t)(cells_x + 1) * (cells_y + 1) * (cells_z + 1);
    hipStream_t s = as_stream(stream);
    ProfScope prof("tsdf_lattice", s);
    MNF_HIP(hipMemsetAsync(counts, 0, 3 * sizeof(int64_t), s));
    hipLaunchKernelGGL(lattice_kernel, dim3(blocks_for(n, kThreads)), dim3(kThreads), 0, s, tsdf, weight, best, n, min_weight, values,
                       reinterpret_cast<unsigned long long *>(counts));
    return launch_status("lattice_kernel");
}

extern "C" int mnf_tsdf_vertex_attrs(const uint32_t *word, const float *best, int32_t cells_x, int32_t cells_y, int32_t cells_z, const double *lo_host,
                                     double voxel, const float *positions, int64_t n, const uint8_t *palette, int32_t n_palette, uint8_t *colour, int32_t *label,
                                     uint8_t *sem_colour, mnf_stream_t stream) {
    MNF_REQUIRE(cells_ok(cells_x, cells_y, cells_z), "tsdf_vertex_attrs: cells per axis must lie in 1 .. %d (got %d x %d x %d)", kMaxCells, cells_x, cells_y,
                cells_z);
    MNF_REQUIRE(lo_host, "tsdf_vertex_attrs: lo_host is null");
    for (int k = 0; k < 3; ++k) MNF_REQUIRE(finite_d(lo_host[k]), "tsdf_vertex_attrs: lo_host[%d] is not finite", k);
    MNF_REQUIRE(positive_d(voxel), "tsdf_vertex_attrs: voxel must be positive and finite (got %g)", voxel);
    MNF_REQUIRE(n >= 0 && n <= 0x7fffffff, "tsdf_vertex_attrs: n outside [0, 2^31) (got %lld)", (long long)n);
    MNF_REQUIRE(word && best, "tsdf_vertex_attrs: a null state array");
    MNF_REQUIRE(aligned4(word) && aligned4(best), "tsdf_vertex_attrs: the state arrays must be 4-byte aligned");
    MNF_REQUIRE(positions || n == 0, "tsdf_vertex_attrs: positions is null");
    MNF_REQUIRE(aligned4(positions) && aligned4(label), "tsdf_vertex_attrs: positions and label must be 4-byte aligned");
    MNF_REQUIRE(n_palette >= 0, "tsdf_vertex_attrs: n_palette is negative (%d)", n_palette);
    MNF_REQUIRE((palette && n_palette > 0) || !sem_colour, "tsdf_vertex_attrs: sem_colour asks for a palette");
    if (n == 0 || (!colour && !label && !sem_colour)) return MNF_OK;
    Cells g = {cells_x, cells_y, cells_z, {lo_host[0], lo_host[1], lo_host[2]}, voxel};
    hipStream_t s = as_stream(stream);
    ProfScope prof("tsdf_vertex_attrs", s);
    hipLaunchKernelGGL(attrs_kernel, dim3(blocks_for(n, kThreads)), dim3(kThreads), 0, s, word, best, g, positions, n, palette, n_palette, colour, label,
                       sem_colour);
    return launch_status("attrs_kernel");
}
