// Scene sensor on the device (gfx950): rgb, planar depth and class views of a labelled, coloured voxel world, what the reference takes from
// habitat_sim (simulator/sim.py:169-196, HabitatSim.sample_images_from_poses).  The definition is in include/mi355nerf.h ("scene sensor");
// tests/sensor_ref.py restates it in numpy.
//   mnf_sensor_build_bricks   one bit per 8 x 8 x 8 brick of the scene: set where a voxel of the brick is occupied
//   mnf_sensor_cast_rays      the walk of the header for given rays
//   mnf_sensor_views          a pixel's ray in the order raygen_kernel forms it (march.hip), the same walk, the shaded bytes
// Built with -ffp-contract=off: a pixel's ray and every step of the walk are chains of separately rounded float64 operations.
//
// The walk.  walk() is the one device function both kernels call.  It steps voxel by voxel: the crossing time of an axis,
// f_a = ((c_a + (step_a > 0)) - g_a) * inv_a, is a function of the integer cell alone, so only the axis that moved forms a new one and the
// other two keep theirs: the same doubles as forming all three every time.  A step touches `voxels` only where the brick's bit is set; in
// empty space it costs the three float64 operations of one axis, the compares and one LDS word.
//
// The brick mask sits in LDS, staged once per workgroup by all of its threads (kMaskWords words at the most: 64 KiB, two workgroups of a
// CU's 160 KiB; a scene of 540 x 84 x 560 voxels takes 6.5 KiB).  A scene whose mask is larger is refused before any HIP call.
//
// views_kernel: a workgroup of 256 threads is a 16 x 16 pixel tile of one view and a wave a 16 x 4 block of it, lane = 16 * row + column.
// Neighbouring pixels walk through the same bricks, so a wave's LDS reads mostly broadcast and its voxel loads share cache lines; every row
// of a wave's rgba and depth stores is one aligned 64-byte run (a pixel's four bytes are one 32-bit store) and its class bytes a 16-byte
// one.  The counts of info are summed per wave by ballot and added with one atomic per wave: integer sums, the same whatever the schedule.
#include "map_dev.h"
#include "pixel_dev.h"

namespace mnf {
namespace {

constexpr int kBrick = 8, kBrickShift = 3;
constexpr int kMaskWords = 16384;                     // 64 KiB of LDS: the budget of a scene's brick mask
constexpr int kThreads = 256;
constexpr int kTile = 16;                             // a workgroup's pixels are kTile x kTile, a wave's kTile x 4
constexpr uint32_t kFreeClass = 0xFFu;
constexpr int kFaceNear = 6, kFaceNone = 255;

struct Scene {
    const uint32_t *voxels;
    int X, Y, Z;
    int BY, BZ;                                       // bricks along y and z
    int mask_words;
    double lo[3], s;
};

struct Shade { uint8_t k[8]; };

inline bool brick_geometry(int32_t X, int32_t Y, int32_t Z, BitGrid *scene, BitGrid *bricks) {
    if (!make_bit_grid(1, X, Y, Z, scene)) return false;
    return make_bit_grid(1, (X + kBrick - 1) >> kBrickShift, (Y + kBrick - 1) >> kBrickShift, (Z + kBrick - 1) >> kBrickShift, bricks);
}

// one thread per run of 8 voxels along z inside one brick: 32 contiguous bytes, one atomic OR where any of them is occupied
__global__ void __launch_bounds__(256) build_bricks_kernel(const uint32_t *__restrict__ voxels, int X, int Y, int Z, int BY, int BZ, int64_t runs,
                                                           uint32_t *__restrict__ bricks) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= runs) return;
    const int bz = (int)(r % BZ);
    const int64_t xy = r / BZ;
    const int y = (int)(xy % Y), x = (int)(xy / Y);
    const int z0 = bz << kBrickShift, z1 = z0 + kBrick < Z ? z0 + kBrick : Z;
    const uint32_t *row = voxels + ((int64_t)x * Y + y) * Z;
    bool any = false;
    for (int z = z0; z < z1; ++z) any = any || (row[z] >> 24) != kFreeClass;
    if (any) {
        const int64_t b = ((int64_t)(x >> kBrickShift) * BY + (y >> kBrickShift)) * BZ + bz;
        atomicOr(bricks + (b >> 5), 1u << (int)(b & 31));
    }
}

__device__ __forceinline__ void stage_mask(const uint32_t *__restrict__ bricks, int words, uint32_t *mask) {
    for (int w = threadIdx.x; w < words; w += kThreads) mask[w] = bricks[w];
    __syncthreads();
}

// The walk of the header.  -> the hit voxel's lin or -1; *t_hit and *face are set on a hit; *bad says the ray was not finite.
__device__ __forceinline__ int walk(const Scene &sc, const uint32_t *mask, const double o[3], const double d[3], double near, double far, double *t_hit,
                                    int *face, bool *bad, uint32_t *word) {
    const int N[3] = {sc.X, sc.Y, sc.Z};
    double g[3], e[3], inv[3];
    int step[3];
    bool finite = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        g[a] = (o[a] - sc.lo[a]) / sc.s;
        e[a] = d[a] / sc.s;
        finite = finite && isfinite(o[a]) && isfinite(d[a]) && isfinite(g[a]) && isfinite(e[a]);
        step[a] = e[a] > 0.0 ? 1 : e[a] < 0.0 ? -1 : 0;
        inv[a] = 1.0 / e[a];
    }
    *bad = !finite;
    if (!finite) return -1;
    double t_in = near, t_out = far;
    int f_in = kFaceNear;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        if (step[a] != 0) {
            const double n = (double)N[a];
            const double t0 = ((step[a] > 0 ? 0.0 : n) - g[a]) * inv[a];
            const double t1 = ((step[a] > 0 ? n : 0.0) - g[a]) * inv[a];
            if (t0 > t_in) { t_in = t0; f_in = 2 * a + (step[a] < 0); }
            if (t1 < t_out) t_out = t1;
        } else if (!(g[a] >= 0.0 && g[a] < (double)N[a])) {
            return -1;
        }
    }
    if (!(t_in <= t_out)) return -1;
    int c[3];
    double f[3];
    const double inf = __longlong_as_double(0x7ff0000000000000ll);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double p = floor(g[a] + e[a] * t_in);
        c[a] = p < 0.0 ? 0 : p > (double)(N[a] - 1) ? N[a] - 1 : (int)p;
        f[a] = step[a] != 0 ? ((double)(c[a] + (step[a] > 0)) - g[a]) * inv[a] : inf;
    }
    double t = t_in;
    int fc = f_in;
    for (;;) {
        const int b = ((c[0] >> kBrickShift) * sc.BY + (c[1] >> kBrickShift)) * sc.BZ + (c[2] >> kBrickShift);
        if ((mask[b >> 5] >> (b & 31)) & 1u) {
            const int lin = (c[0] * sc.Y + c[1]) * sc.Z + c[2];
            const uint32_t w = sc.voxels[lin];
            if ((w >> 24) != kFreeClass) {
                *t_hit = t > t_in ? t : t_in;
                *face = fc;
                *word = w;
                return lin;
            }
        }
        int a = 0;
        if (f[1] < f[a]) a = 1;
        if (f[2] < f[a]) a = 2;
        const double fa = a == 0 ? f[0] : a == 1 ? f[1] : f[2];
        if (!(fa <= t_out)) return -1;
        // one select per axis keeps the arrays in registers
        const int sa = a == 0 ? step[0] : a == 1 ? step[1] : step[2];
        const int ca = (a == 0 ? c[0] : a == 1 ? c[1] : c[2]) + sa;
        const int na = a == 0 ? N[0] : a == 1 ? N[1] : N[2];
        if ((unsigned)ca >= (unsigned)na) return -1;
        const double ga = a == 0 ? g[0] : a == 1 ? g[1] : g[2], ia = a == 0 ? inv[0] : a == 1 ? inv[1] : inv[2];
        const double fn = ((double)(ca + (sa > 0)) - ga) * ia;
        c[0] = a == 0 ? ca : c[0]; c[1] = a == 1 ? ca : c[1]; c[2] = a == 2 ? ca : c[2];
        f[0] = a == 0 ? fn : f[0]; f[1] = a == 1 ? fn : f[1]; f[2] = a == 2 ? fn : f[2];
        t = fa;
        fc = 2 * a + (sa < 0);
    }
}

__device__ __forceinline__ void count_info(bool miss, bool bad, unsigned long long *info) {
    const unsigned long long m = __ballot(miss), b = __ballot(bad);
    if ((threadIdx.x & 63) == 0) {
        if (m) atomicAdd(info, (unsigned long long)__popcll(m));
        if (b) atomicAdd(info + 1, (unsigned long long)__popcll(b));
    }
}

__global__ void __launch_bounds__(kThreads) cast_kernel(Scene sc, const uint32_t *__restrict__ bricks, const double *__restrict__ origins,
                                                        const double *__restrict__ dirs, int64_t n, double near, double far, double *__restrict__ t_hit,
                                                        int32_t *__restrict__ hit, uint8_t *__restrict__ face, unsigned long long *__restrict__ info) {
    extern __shared__ uint32_t mask[];
    stage_mask(bricks, sc.mask_words, mask);
    const int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const bool live = r < n;
    int lin = -1, fc = kFaceNone;
    double t = -1.0;
    bool bad = false;
    if (live) {
        const double o[3] = {origins[3 * r], origins[3 * r + 1], origins[3 * r + 2]};
        const double d[3] = {dirs[3 * r], dirs[3 * r + 1], dirs[3 * r + 2]};
        uint32_t word;
        double th;
        int f;
        lin = walk(sc, mask, o, d, near, far, &th, &f, &bad, &word);
        if (lin >= 0) { t = th; fc = f; }
        t_hit[r] = t;
        hit[r] = lin;
        face[r] = (uint8_t)fc;
    }
    count_info(live && lin < 0, live && bad, info);
}

__global__ void __launch_bounds__(kThreads) views_kernel(Scene sc, const uint32_t *__restrict__ bricks, const double *__restrict__ c2w, int W, int H,
                                                         int tiles_x, int tiles_y, double focal, double near, double far, int ray_depth, Shade shade,
                                                         uint32_t background, uint32_t *__restrict__ rgba, float *__restrict__ depth,
                                                         uint8_t *__restrict__ sem, int32_t *__restrict__ hit, unsigned long long *__restrict__ info) {
    extern __shared__ uint32_t mask[];
    stage_mask(bricks, sc.mask_words, mask);
    const int tile = blockIdx.x % (tiles_x * tiles_y);
    const int64_t v = blockIdx.x / (tiles_x * tiles_y);
    const int tx = tile % tiles_x, ty = tile / tiles_x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int x = tx * kTile + (lane & 15), y = ty * kTile + wave * 4 + (lane >> 4);
    const bool live = x < W && y < H;
    int lin = -1;
    bool bad = false;
    if (live) {
        const double *m = c2w + v * 12;
        double cam0, cam1, d[3];
        pixel_ray(x, y, W, H, focal, m, cam0, cam1, d);
        const double o[3] = {m[3], m[7], m[11]};
        uint32_t word = 0;
        double t = 0.0;
        int fc = kFaceNear;
        lin = walk(sc, mask, o, d, near, far, &t, &fc, &bad, &word);
        const int64_t p = (v * H + y) * W + x;
        uint32_t px = background;
        float dep = 0.0f;
        uint8_t cls = 0;
        if (lin >= 0) {
            const uint32_t k = shade.k[fc];
            const uint32_t r = ((word & 0xFFu) * k + 127u) / 255u, gr = (((word >> 8) & 0xFFu) * k + 127u) / 255u, b = (((word >> 16) & 0xFFu) * k + 127u) / 255u;
            px = r | (gr << 8) | (b << 16) | 0xFF000000u;
            dep = ray_depth ? (float)(t * sqrt((cam0 * cam0 + cam1 * cam1) + 1.0)) : (float)t;
            cls = (uint8_t)(word >> 24);
        }
        rgba[p] = px;
        depth[p] = dep;
        sem[p] = cls;
        if (hit) hit[p] = lin;
    }
    count_info(live && lin < 0, live && bad, info);
}

int scene_arguments(const char *who, const uint32_t *voxels, int32_t X, int32_t Y, int32_t Z, const uint32_t *bricks, const double *lo_host, double s,
                    double near, double far, const int64_t *info, Scene *sc) {
    BitGrid grid, bg;
    MNF_REQUIRE(X > 0 && Y > 0 && Z > 0, "%s: sizes must be positive (got %d x %d x %d)", who, X, Y, Z);
    MNF_REQUIRE(brick_geometry(X, Y, Z, &grid, &bg), "%s: %d x %d x %d voxels are outside the limits of a bit grid", who, X, Y, Z);
    MNF_REQUIRE(bg.wpp <= kMaskWords, "%s: the brick mask of %d x %d x %d voxels takes %lld words, more than the %d (64 KiB of LDS) a workgroup stages", who, X,
                Y, Z, (long long)bg.wpp, kMaskWords);
    MNF_REQUIRE(lo_host, "%s: lo_host is null", who);
    for (int k = 0; k < 3; ++k) MNF_REQUIRE(finite_d(lo_host[k]), "%s: lo_host[%d] is not finite", who, k);
    MNF_REQUIRE(s > 0.0 && s <= 1.79e308, "%s: the voxel size must be positive and finite (got %g)", who, s);
    MNF_REQUIRE(near >= 0.0 && far >= near && far <= 1.79e308, "%s: need 0 <= near <= far, far finite (got %g, %g)", who, near, far);
    MNF_REQUIRE(info, "%s: info is null", who);
    MNF_REQUIRE(aligned8(info), "%s: info must be 8-byte aligned", who);
    MNF_REQUIRE(voxels && bricks, "%s: a null scene pointer", who);
    MNF_REQUIRE(aligned4(voxels) && aligned4(bricks), "%s: voxels and bricks must be 4-byte aligned", who);
    *sc = {voxels, X, Y, Z, bg.Y, bg.Z, (int)bg.wpp, {lo_host[0], lo_host[1], lo_host[2]}, s};
    return MNF_OK;
}

}  // namespace
}  // namespace mnf

using namespace mnf;

extern "C" int64_t mnf_sensor_bricks_words(int32_t X, int32_t Y, int32_t Z) {
    BitGrid grid, bg;
    if (!brick_geometry(X, Y, Z, &grid, &bg) || bg.wpp > kMaskWords) return -1;
    return bg.wpp;
}

extern "C" int mnf_sensor_build_bricks(const uint32_t *voxels, int32_t X, int32_t Y, int32_t Z, uint32_t *bricks, mnf_stream_t stream) {
    BitGrid grid, bg;
    MNF_REQUIRE(X > 0 && Y > 0 && Z > 0, "sensor_build_bricks: sizes must be positive (got %d x %d x %d)", X, Y, Z);
    MNF_REQUIRE(brick_geometry(X, Y, Z, &grid, &bg), "sensor_build_bricks: %d x %d x %d voxels are outside the limits of a bit grid", X, Y, Z);
    MNF_REQUIRE(bg.wpp <= kMaskWords, "sensor_build_bricks: the brick mask of %d x %d x %d voxels takes %lld words, more than %d (64 KiB of LDS)", X, Y, Z,
                (long long)bg.wpp, kMaskWords);
    MNF_REQUIRE(voxels && bricks, "sensor_build_bricks: a null pointer");
    MNF_REQUIRE(aligned4(voxels) && aligned4(bricks),
                "sensor_build_bricks: voxels and bricks must be 4-byte aligned");
    hipStream_t s = as_stream(stream);
    ProfScope prof("sensor_build_bricks", s);
    MNF_HIP(hipMemsetAsync(bricks, 0, (size_t)bg.wpp * sizeof(uint32_t), s));
    const int64_t runs = (int64_t)X * Y * bg.Z;
    hipLaunchKernelGGL(build_bricks_kernel, dim3(blocks_for(runs)), dim3(256), 0, s, voxels, X, Y, Z, bg.Y, bg.Z, runs, bricks);
    return launch_status("build_bricks_kernel");
}

extern "C" int mnf_sensor_cast_rays(const uint32_t *voxels, int32_t X, int32_t Y, int32_t Z, const uint32_t *bricks, const double *lo_host, double voxel_size,
                                    const double *origins, const double *dirs, int64_t n, double near, double far, double *t_hit, int32_t *hit, uint8_t *face,
                                    int64_t *info, mnf_stream_t stream) {
    Scene sc;
    const int rc = scene_arguments("sensor_cast_rays", voxels, X, Y, Z, bricks, lo_host, voxel_size, near, far, info, &sc);
    if (rc != MNF_OK) return rc;
    MNF_REQUIRE(n >= 0 && n <= (int64_t)0x7fffffff * kThreads, "sensor_cast_rays: n outside what one launch holds (%lld)", (long long)n);
    MNF_REQUIRE((origins && dirs && t_hit && hit && face) || n == 0, "sensor_cast_rays: a null ray or output array");
    MNF_REQUIRE(aligned8(origins) && aligned8(dirs) && aligned8(t_hit), "sensor_cast_rays: origins, dirs and t_hit must be 8-byte aligned");
    MNF_REQUIRE(aligned4(hit), "sensor_cast_rays: hit must be 4-byte aligned");
    if (n == 0) return MNF_OK;
    hipStream_t s = as_stream(stream);
    ProfScope prof("sensor_cast_rays", s);
    hipLaunchKernelGGL(cast_kernel, dim3(blocks_for(n, kThreads)), dim3(kThreads), (size_t)sc.mask_words * sizeof(uint32_t), s, sc, bricks, origins, dirs, n, near,
                       far, t_hit, hit, face, reinterpret_cast<unsigned long long *>(info));
    return launch_status("cast_kernel");
}

extern "C" int mnf_sensor_views(const uint32_t *voxels, int32_t X, int32_t Y, int32_t Z, const uint32_t *bricks, const double *lo_host, double voxel_size,
                                const double *c2w, int32_t n_views, int32_t width, int32_t height, double focal, double near, double far, int32_t depth_mode,
                                const uint8_t *shade_host, uint32_t background, uint8_t *rgba, float *depth, uint8_t *sem, int32_t *hit, int64_t *info,
                                mnf_stream_t stream) {
    Scene sc;
    const int rc = scene_arguments("sensor_views", voxels, X, Y, Z, bricks, lo_host, voxel_size, near, far, info, &sc);
    if (rc != MNF_OK) return rc;
    MNF_REQUIRE(n_views >= 0, "sensor_views: n_views is negative (%d)", n_views);
    MNF_REQUIRE(width > 0 && height > 0 && width <= 16384 && height <= 16384, "sensor_views: the image is %d x %d (1 .. 16384 each)", width, height);
    MNF_REQUIRE(focal > 0.0 && focal <= 1.79e308, "sensor_views: focal must be positive and finite (got %g)", focal);
    MNF_REQUIRE(depth_mode == MNF_SENSOR_DEPTH_PLANAR || depth_mode == MNF_SENSOR_DEPTH_RAY, "sensor_views: depth_mode %d is neither planar nor ray", depth_mode);
    MNF_REQUIRE(shade_host, "sensor_views: shade_host is null");
    const int tiles_x = (width + kTile - 1) / kTile, tiles_y = (height + kTile - 1) / kTile;
    const int64_t blocks = (int64_t)tiles_x * tiles_y * n_views;
    MNF_REQUIRE(blocks <= 0x7fffffff, "sensor_views: %d views of %d x %d are more than one launch holds", n_views, width, height);
    MNF_REQUIRE((c2w && rgba && depth && sem) || n_views == 0, "sensor_views: a null pose or output array");
    MNF_REQUIRE(aligned8(c2w), "sensor_views: c2w must be 8-byte aligned");
    MNF_REQUIRE(aligned4(rgba) && aligned4(depth) && aligned4(hit),
                "sensor_views: rgba, depth and hit must be 4-byte aligned");
    if (n_views == 0) return MNF_OK;
    Shade shade;
    for (int k = 0; k < 7; ++k) shade.k[k] = shade_host[k];
    shade.k[7] = 0;
    hipStream_t s = as_stream(stream);
    ProfScope prof("sensor_views", s);
    hipLaunchKernelGGL(views_kernel, dim3((unsigned)blocks), dim3(kThreads), (size_t)sc.mask_words * sizeof(uint32_t), s, sc, bricks, c2w, width, height, tiles_x,
                       tiles_y, focal, near, far, depth_mode == MNF_SENSOR_DEPTH_RAY, shade, background, reinterpret_cast<uint32_t *>(rgba), depth, sem, hit,
                       reinterpret_cast<unsigned long long *>(info));
    return launch_status("views_kernel");
}
