// Trajectory clearance on the device (gfx950): the exact squared distance field of the ensemble's occupancy grids, trajectory samples
// looked up in it, and the reference's voxel walk.
//   mnf_clearance_field   the Euclidean distance transform the reference has no counterpart of (its planner dilates one slice by a 3 x 3 box)
//   mnf_clearance_lookup  <- planning/planning_funcs.py:187-189 (world2voxels: numpy's float64 floor_divide, restated in full below)
//   mnf_voxel_walk_*      <- planning/planning_funcs.py:97-159 (get_voxels_between_points), :162-179 (collision_checker's clipped look-up)
// Built with -ffp-contract=off: a voxel index and every step of a walk are chains of separately rounded float64 operations.
//
// The field is separable: g0[v] = 0 where a member holds the voxel, kFar elsewhere, and along each axis in turn (z, then y, then x)
//   g'[i] = min_j (i - j)^2 + g[j].
// All values are integers, min and + are exact, so the result is the brute-force answer and the same bytes every time.  kFar = 2^30: a
// finite value is at most 3 * 2047^2 < 2^24 and kFar + 2047^2 < 2^31, so no sum wraps; whatever is >= kFar after the last pass had no
// occupied voxel anywhere and is written as INT32_MAX.
//
// edt_pass_kernel, one workgroup of 256 threads per tile, the tile's lines in dynamic LDS, one output per thread and turn.  The estimator's
// layout is lin = (x Y + y) Z + z, so the volume is [A][n][B] for the axis under way: n its extent, B the stride of a step along it.
//   along z  (B = 1): a tile is `lines` whole lines, which lie back to back: one contiguous run of lines * n values, loaded and stored in order.
//   along y, x (B > 1): a tile is all n values of `lines` neighbouring columns b: LDS [n][lines], every row of it a contiguous run in memory,
//            so the loads and stores of all three passes run along z.  lines = 64 while n * 64 words fit 64 KiB, else 32, 16, 8 (n = 2048).
// Thread o of a turn owns the tile's value o (the LDS word o: the tile is laid out as its memory is), and looks outwards from it: the
// candidates at distance k, k = 1, 2, ..., while k * k is below the best so far and a candidate exists; a farther j cannot win since
// (i - j)^2 alone is no less than the best.  The lanes of a wave own consecutive words and look at the same k, so every ds_read_b32 of the
// loop reads 64 consecutive words (one per bank pair, conflict-free); on an empty line the loop runs to the line's end, n - 1 steps at most.
// A pass works in place: a tile is read whole into LDS before a barrier and written after it, and tiles are disjoint.
// The last pass also counts the occupied voxels and takes the largest finite value: integer atomics, the same whatever the schedule.
//
// lookup_kernel: one workgroup per trajectory; every sample's voxel, its field value, and the least (value << 32 | index) of the workgroup.
// walk kernels: one lane per walk, every walk bounded by the caller's max_steps.
#include "map_dev.h"

namespace mnf {
namespace {

constexpr int kEdtThreads = 256;
constexpr int kFar = 1 << 30;
constexpr int kMaxFieldAxis = 2048;
constexpr int kTileWords = 16384;                     // 64 KiB of LDS at the most
constexpr int kLineRun = 4096;                        // values of one tile of the pass along z (a longer line is a tile of its own: n <= 2048)
constexpr int kCellFar = 1 << 30;                     // a voxel index is clamped to +-2^30; INT32_MIN stands for "not finite"

inline bool field_geometry_ok(int32_t n_members, int32_t X, int32_t Y, int32_t Z, BitGrid *g) {
    if (X > kMaxFieldAxis || Y > kMaxFieldAxis || Z > kMaxFieldAxis) return false;
    return make_bit_grid(n_members, X, Y, Z, g);
}

// kFirst: the values come from the members' bytes.  kLast: kFar becomes INT32_MAX and the two numbers of info are formed.
// tile_lines, n, B as above; `count` = the volume's values (the run of the z pass is clipped to it).
template <bool kFirst, bool kLast>
__global__ void __launch_bounds__(kEdtThreads) edt_pass_kernel(const uint8_t *__restrict__ binaries, int n_members, int64_t count, int32_t *d2, int n, int64_t B,
                                                               int tile_lines, long long *__restrict__ info) {
    extern __shared__ int32_t g[];
    const int tid = threadIdx.x;
    const bool run = B == 1;                          // (uniform) the pass along z
    const int words = tile_lines * n;
    const int step = run ? 1 : tile_lines;            // LDS words between neighbours along the axis
    int64_t base;                                     // of the tile in memory
    int valid;                                        // run: values of the tile inside the volume; else: columns of the tile inside B
    if (run) {
        base = (int64_t)blockIdx.x * words;
        const int64_t left = count - base;
        valid = left < words ? (int)left : words;
    } else {
        const int64_t b0 = (int64_t)blockIdx.x * tile_lines;
        base = (int64_t)blockIdx.y * n * B + b0;
        const int64_t left = B - b0;
        valid = left < tile_lines ? (int)left : tile_lines;
    }
    for (int o = tid; o < words; o += kEdtThreads) {
        int v = kFar;
        int64_t at = -1;
        if (run) { if (o < valid) at = base + o; }
        else { const int i = o / tile_lines, q = o - i * tile_lines; if (q < valid) at = base + (int64_t)i * B + q; }
        if (at >= 0) {
            if (kFirst) {
                bool any = false;
                for (int m = 0; m < n_members; ++m) any = any || binaries[(int64_t)m * count + at] != 0;
                v = any ? 0 : kFar;
            } else {
                v = d2[at];
            }
        }
        g[o] = v;
    }
    __syncthreads();
    long long occupied = 0;
    int largest = -1;
    for (int o = tid; o < words; o += kEdtThreads) {
        int64_t at = -1;
        int i;
        if (run) { i = o % n; if (o < valid) at = base + o; }
        else { i = o / tile_lines; const int q = o - i * tile_lines; if (q < valid) at = base + (int64_t)i * B + q; }
        if (at < 0) continue;
        int best = g[o];
        const int reach = i > n - 1 - i ? i : n - 1 - i;
        for (int k = 1; k <= reach && k * k < best; ++k) {
            const int kk = k * k;
            if (k <= i) { const int c = g[o - k * step] + kk; best = c < best ? c : best; }
            if (k <= n - 1 - i) { const int c = g[o + k * step] + kk; best = c < best ? c : best; }
        }
        if (kLast) {
            if (best >= kFar) best = 0x7fffffff;
            else { occupied += best == 0; largest = best > largest ? best : largest; }
        }
        d2[at] = best;
    }
    if (kLast) {
        occupied = wave_sum(occupied);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const int other = __shfl_down(largest, off, 64);
            largest = other > largest ? other : largest;
        }
        if ((tid & 63) == 0) {
            if (occupied) atomicAdd(reinterpret_cast<unsigned long long *>(info), (unsigned long long)occupied);
            if (largest >= 0) atomicMax(info + 1, (long long)largest);
        }
    }
}

__global__ void field_info_init_kernel(long long *info) { info[0] = 0; info[1] = -1; }

// ---------------------------------------------------------------------------------------------------------------- voxel of a point
// numpy's float64 floor_divide (npy_divmod): the exact remainder, the sign fix, the round-up of a quotient that lies just below an integer.
__device__ __forceinline__ double np_floor_divide(double a, double b) {
    if (b == 0.0) return a / b;
    double mod = fmod(a, b);
    double div = (a - mod) / b;
    if (mod != 0.0) {
        if ((b < 0.0) != (mod < 0.0)) div -= 1.0;
    }
    double fl;
    if (div != 0.0) {
        fl = floor(div);
        if (div - fl > 0.5) fl += 1.0;
    } else {
        fl = copysign(0.0, a / b);
    }
    return fl;
}

__device__ __forceinline__ int cell_of(double f) {
    if (!isfinite(f)) return (int)0x80000000;
    return f > (double)kCellFar ? kCellFar : f < -(double)kCellFar ? -kCellFar : (int)f;
}

constexpr int kLookupThreads = 256;

__global__ void __launch_bounds__(kLookupThreads) lookup_kernel(const int32_t *__restrict__ d2, int X, int Y, int Z, double ox, double oy, double oz, double voxel,
                                                                const double *__restrict__ points, int64_t n_points, const int64_t *__restrict__ offsets,
                                                                int32_t *__restrict__ cells, int32_t *__restrict__ point_d2, long long *__restrict__ traj,
                                                                unsigned long long *__restrict__ info) {
    __shared__ unsigned long long wave_key[kLookupThreads / 64];
    __shared__ int wave_out[kLookupThreads / 64], wave_bad[kLookupThreads / 64];
    const int tid = threadIdx.x;
    const int64_t t = blockIdx.x;
    int64_t first = offsets[t], last = offsets[t + 1];
    first = first < 0 ? 0 : first > n_points ? n_points : first;                      // nothing outside the arrays is touched, whatever the offsets hold
    last = last < first ? first : last > n_points ? n_points : last;
    unsigned long long key = ~0ull;
    int outside = 0, bad = 0;
    for (int64_t p = first + tid; p < last; p += kLookupThreads) {
        const double x = points[3 * p], y = points[3 * p + 1], z = points[3 * p + 2];
        const int cx = cell_of(np_floor_divide(x - ox, voxel)), cy = cell_of(np_floor_divide(y - oy, voxel)), cz = cell_of(np_floor_divide(z - oz, voxel));
        cells[3 * p] = cx; cells[3 * p + 1] = cy; cells[3 * p + 2] = cz;
        int v = -1;
        if (!(isfinite(x) && isfinite(y) && isfinite(z))) { ++bad; ++outside; }
        else if ((unsigned)cx >= (unsigned)X || (unsigned)cy >= (unsigned)Y || (unsigned)cz >= (unsigned)Z) ++outside;
        else {
            v = d2[((int64_t)cx * Y + cy) * Z + cz];
            const unsigned long long k = ((unsigned long long)(unsigned)v << 32) | (unsigned long long)(p - first);
            key = k < key ? k : key;
        }
        point_d2[p] = v;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long other = __shfl_down(key, off, 64);
        key = other < key ? other : key;
    }
    wave_sum_each(outside, bad);
    if ((tid & 63) == 0) { wave_key[tid >> 6] = key; wave_out[tid >> 6] = outside; wave_bad[tid >> 6] = bad; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < kLookupThreads / 64; ++w) {
            key = wave_key[w] < key ? wave_key[w] : key;
            outside += wave_out[w];
            bad += wave_bad[w];
        }
        long long *row = traj + 4 * t;
        row[0] = key == ~0ull ? -1 : (long long)(key >> 32);
        row[1] = key == ~0ull ? -1 : (long long)(key & 0xffffffffull);
        row[2] = outside;
        row[3] = last - first;
        if (outside) atomicAdd(info, (unsigned long long)outside);
        if (bad) atomicAdd(info + 1, (unsigned long long)bad);
    }
}

// ---------------------------------------------------------------------------------------------------------------- the voxel walk
// get_voxels_between_points, statement by statement; `visit(k, x, y, z)` sees the k-th listed voxel and returns false to end the walk early.
// -> the length of the list (cut at max_steps; *cut says so), or -1 for an input that is not finite.
template <typename Visit>
__device__ __forceinline__ long long walk(const double *__restrict__ start, const double *__restrict__ end, const int32_t *__restrict__ cur0,
                                          const int32_t *__restrict__ end_voxel, double size, long long max_steps, bool *cut, Visit visit) {
    double t_max[3], t_delta[3], stepf[3];
    int cur[3], view[3], stepi[3], last[3];
    bool finite = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double s = start[a], e = end[a];
        finite = finite && isfinite(s) && isfinite(e);
        const double ray = e - s;
        cur[a] = view[a] = cur0[a];
        last[a] = end_voxel[a];
        stepi[a] = ray >= 0.0 ? 1 : -1;
        stepf[a] = (double)stepi[a];
        const double next = ((double)cur[a] + stepf[a]) * size;
        const double inf = __longlong_as_double(0x7ff0000000000000ll);
        t_max[a] = ray != 0.0 ? (next - s) / ray : inf;
        t_delta[a] = ray != 0.0 ? size / ray * stepf[a] : inf;
    }
    *cut = false;
    if (!finite) return -1;
    double r[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) { const double d = (double)(int)((unsigned)last[a] - (unsigned)view[a]) * size; r[a] = d * d; }
    const double range_sq = (r[0] + r[1]) + r[2];
    double dist = 0.0;
    long long n = 0;
    while (dist <= range_sq) {
        if (n >= max_steps) { *cut = true; break; }
        int a;
        if (t_max[0] < t_max[1]) a = t_max[0] < t_max[2] ? 0 : 2;
        else a = t_max[1] < t_max[2] ? 1 : 2;
        // one select per axis keeps the three arrays in registers
        cur[0] = (int)((unsigned)cur[0] + (a == 0 ? (unsigned)stepi[0] : 0u));
        cur[1] = (int)((unsigned)cur[1] + (a == 1 ? (unsigned)stepi[1] : 0u));
        cur[2] = (int)((unsigned)cur[2] + (a == 2 ? (unsigned)stepi[2] : 0u));
        t_max[0] = a == 0 ? t_max[0] + t_delta[0] : t_max[0];
        t_max[1] = a == 1 ? t_max[1] + t_delta[1] : t_max[1];
        t_max[2] = a == 2 ? t_max[2] + t_delta[2] : t_max[2];
        const bool more = visit(n, cur[0], cur[1], cur[2]);
        ++n;
        if (!more) break;
#pragma unroll
        for (int b = 0; b < 3; ++b) { const double d = (double)(int)((unsigned)cur[b] - (unsigned)view[b]) * size; r[b] = d * d; }
        dist = (r[0] + r[1]) + r[2];
    }
    return n;
}

__global__ void __launch_bounds__(256) walk_count_kernel(const double *__restrict__ start, const double *__restrict__ end, const int32_t *__restrict__ cur,
                                                         const int32_t *__restrict__ end_voxel, int64_t n, double size, long long max_steps,
                                                         long long *__restrict__ counts, unsigned long long *__restrict__ info) {
    const int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (w >= n) return;
    bool cut;
    const long long len = walk(start + 3 * w, end + 3 * w, cur + 3 * w, end_voxel + 3 * w, size, max_steps, &cut, [](long long, int, int, int) { return true; });
    counts[w] = len < 0 ? 0 : len;
    if (cut) atomicAdd(info, 1ull);
    if (len < 0) atomicAdd(info + 1, 1ull);
}

__global__ void __launch_bounds__(256) walk_fill_kernel(const double *__restrict__ start, const double *__restrict__ end, const int32_t *__restrict__ cur,
                                                        const int32_t *__restrict__ end_voxel, int64_t n, double size, long long max_steps,
                                                        const int64_t *__restrict__ offsets, int64_t total, int32_t *__restrict__ voxels,
                                                        unsigned long long *__restrict__ info) {
    const int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (w >= n) return;
    const int64_t first = offsets[w], slot = offsets[w + 1] - first;
    const bool room = first >= 0 && slot >= 0 && first <= total && slot <= total - first;
    const long long cap = room ? slot : 0;                                            // nothing is written past the slot, or outside `voxels`
    bool cut;
    int32_t *out = voxels + 3 * (room ? first : 0);
    const long long len = walk(start + 3 * w, end + 3 * w, cur + 3 * w, end_voxel + 3 * w, size, max_steps, &cut, [out, cap](long long k, int x, int y, int z) {
        if (k < cap) { out[3 * k] = x; out[3 * k + 1] = y; out[3 * k + 2] = z; }
        return true;
    });
    if (cut) atomicAdd(info, 1ull);
    if (len < 0) atomicAdd(info + 1, 1ull);
    if (!room || (len < 0 ? 0 : len) != slot) atomicAdd(info + 2, 1ull);              // not the slot mnf_voxel_walk_count sized
}

__global__ void __launch_bounds__(256) walk_hits_kernel(const double *__restrict__ start, const double *__restrict__ end, const int32_t *__restrict__ cur,
                                                        const int32_t *__restrict__ end_voxel, int64_t n, double size, long long max_steps,
                                                        const uint8_t *__restrict__ binaries, int n_members, int X, int Y, int Z,
                                                        int32_t *__restrict__ hits, unsigned long long *__restrict__ info) {
    const int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (w >= n) return;
    const int64_t count = (int64_t)X * Y * Z;
    int at = -1, hx = -1, hy = -1, hz = -1;
    bool cut;
    const long long len = walk(start + 3 * w, end + 3 * w, cur + 3 * w, end_voxel + 3 * w, size, max_steps, &cut,
                               [&](long long k, int x, int y, int z) {
                                   if (at >= 0) return true;                          // the walk goes on: its length is part of the row
                                   const int cx = x < 0 ? 0 : x > X - 1 ? X - 1 : x, cy = y < 0 ? 0 : y > Y - 1 ? Y - 1 : y, cz = z < 0 ? 0 : z > Z - 1 ? Z - 1 : z;
                                   const int64_t lin = ((int64_t)cx * Y + cy) * Z + cz;
                                   bool any = false;
                                   for (int m = 0; m < n_members; ++m) any = any || binaries[(int64_t)m * count + lin] != 0;
                                   if (any) { at = (int)k; hx = x; hy = y; hz = z; }
                                   return true;
                               });
    int32_t *row = hits + 5 * w;
    row[0] = at; row[1] = hx; row[2] = hy; row[3] = hz; row[4] = (int)(len < 0 ? 0 : len);
    if (cut) atomicAdd(info, 1ull);
    if (len < 0) atomicAdd(info + 1, 1ull);
}

int walk_arguments(const char *who, const double *start, const double *end, const int32_t *cur, const int32_t *end_voxel, int64_t n, double size, int64_t max_steps,
                   const int64_t *info) {
    MNF_REQUIRE(n >= 0, "%s: n is negative (%lld)", who, (long long)n);
    MNF_REQUIRE(n <= (int64_t)0x7fffffff * 256, "%s: n is more than one launch holds (%lld)", who, (long long)n);
    MNF_REQUIRE(size > 0.0 && size <= 1.79e308, "%s: voxel_size must be positive and finite (got %g)", who, size);
    MNF_REQUIRE(max_steps >= 0 && max_steps <= 0x7fffffff, "%s: max_steps outside [0, 2^31) (%lld)", who, (long long)max_steps);
    MNF_REQUIRE(info, "%s: info is null", who);
    MNF_REQUIRE(aligned8(info), "%s: info must be 8-byte aligned", who);
    MNF_REQUIRE((start && end && cur && end_voxel) || n == 0, "%s: a null position or voxel array", who);
    MNF_REQUIRE(aligned8(start) && aligned8(end), "%s: positions must be 8-byte aligned", who);
    return MNF_OK;
}

}  // namespace
}  // namespace mnf

using namespace mnf;

extern "C" int mnf_clearance_field(const uint8_t *binaries, int32_t n_members, int32_t X, int32_t Y, int32_t Z, int32_t *d2, int64_t *info,
                                   mnf_stream_t stream) {
    BitGrid grid;
    MNF_REQUIRE(X > 0 && Y > 0 && Z > 0 && n_members > 0, "clearance_field: sizes must be positive (got %d members of %d x %d x %d)", n_members, X, Y, Z);
    MNF_REQUIRE(field_geometry_ok(n_members, X, Y, Z, &grid), "clearance_field: %d members of %d x %d x %d are outside the limits (axes <= %d, < 2^31 - 64 voxels)",
                n_members, X, Y, Z, kMaxFieldAxis);
    MNF_REQUIRE(binaries && d2 && info, "clearance_field: a null pointer");
    MNF_REQUIRE(aligned8(info), "clearance_field: info must be 8-byte aligned");
    hipStream_t s = as_stream(stream);
    ProfScope prof("clearance_field", s);
    long long *inf = reinterpret_cast<long long *>(info);
    hipLaunchKernelGGL(field_info_init_kernel, dim3(1), dim3(1), 0, s, inf);
    const int64_t count = grid.n_vox;
    // the pass along z always runs (it reads the members' bytes); an axis of one voxel has no pass; the last one that runs forms info
    struct Pass { int n; int64_t B; int A; } passes[3];
    int n_passes = 0;
    passes[n_passes++] = {Z, 1, 1};
    if (Y > 1) passes[n_passes++] = {Y, (int64_t)Z, X};
    if (X > 1) passes[n_passes++] = {X, (int64_t)Y * Z, 1};
    for (int p = 0; p < n_passes; ++p) {
        const Pass &ps = passes[p];
        const bool first = p == 0, last = p == n_passes - 1;
        int lines;
        dim3 blocks;
        if (ps.B == 1) {                                                              // lines back to back (along z, or the axes after it have one voxel)
            lines = ps.n >= kLineRun ? 1 : kLineRun / ps.n;
            blocks = dim3((unsigned)ceil_div(count, (int64_t)lines * ps.n));
        } else {
            lines = 64;
            while ((int64_t)lines * ps.n > kTileWords) lines >>= 1;
            blocks = dim3((unsigned)ceil_div(ps.B, lines), (unsigned)ps.A);
        }
        const size_t lds = (size_t)lines * ps.n * sizeof(int32_t);
        auto kernel = first ? (last ? edt_pass_kernel<true, true> : edt_pass_kernel<true, false>) : (last ? edt_pass_kernel<false, true> : edt_pass_kernel<false, false>);
        hipLaunchKernelGGL(kernel, blocks, dim3(kEdtThreads), lds, s, binaries, n_members, count, d2, ps.n, ps.B, lines, inf);
    }
    return launch_status("edt_pass_kernel");
}

extern "C" int mnf_clearance_lookup(const int32_t *d2, int32_t X, int32_t Y, int32_t Z, const double *origin_host, double voxel, const double *points,
                                    int64_t n_points, const int64_t *offsets, int64_t n_traj, int32_t *cells, int32_t *point_d2, int64_t *traj, int64_t *info,
                                    mnf_stream_t stream) {
    BitGrid grid;
    MNF_REQUIRE(X > 0 && Y > 0 && Z > 0, "clearance_lookup: sizes must be positive (got %d x %d x %d)", X, Y, Z);
    MNF_REQUIRE(field_geometry_ok(1, X, Y, Z, &grid), "clearance_lookup: %d x %d x %d is outside the limits of a clearance field", X, Y, Z);
    MNF_REQUIRE(origin_host, "clearance_lookup: origin_host is null");
    MNF_REQUIRE(voxel > 0.0 && voxel <= 1.79e308, "clearance_lookup: voxel must be positive and finite (got %g)", voxel);
    for (int k = 0; k < 3; ++k) MNF_REQUIRE(finite_d(origin_host[k]), "clearance_lookup: origin_host[%d] is not finite", k);
    MNF_REQUIRE(n_points >= 0 && n_points < ((int64_t)1 << 31), "clearance_lookup: n_points outside [0, 2^31) (%lld)", (long long)n_points);
    MNF_REQUIRE(n_traj >= 0 && n_traj < ((int64_t)1 << 31), "clearance_lookup: n_traj outside [0, 2^31) (%lld)", (long long)n_traj);
    MNF_REQUIRE(info, "clearance_lookup: info is null");
    MNF_REQUIRE(aligned8(info) && aligned8(traj) && aligned8(offsets) && aligned8(points), "clearance_lookup: points, offsets, traj and info must be 8-byte aligned");
    if (n_traj == 0) return MNF_OK;
    MNF_REQUIRE(d2 && offsets && traj, "clearance_lookup: a null pointer");
    MNF_REQUIRE((points && cells && point_d2) || n_points == 0, "clearance_lookup: a null point array");
    hipStream_t s = as_stream(stream);
    ProfScope prof("clearance_lookup", s);
    hipLaunchKernelGGL(lookup_kernel, dim3((unsigned)n_traj), dim3(kLookupThreads), 0, s, d2, X, Y, Z, origin_host[0], origin_host[1], origin_host[2], voxel, points,
                       n_points, offsets, cells, point_d2, reinterpret_cast<long long *>(traj), reinterpret_cast<unsigned long long *>(info));
    return launch_status("lookup_kernel");
}

extern "C" int mnf_voxel_walk_count(const double *start, const double *end, const int32_t *current_voxel, const int32_t *end_voxel, int64_t n, double voxel_size,
                                    int64_t max_steps, int64_t *counts, int64_t *info, mnf_stream_t stream) {
    const int rc = walk_arguments("voxel_walk_count", start, end, current_voxel, end_voxel, n, voxel_size, max_steps, info);
    if (rc != MNF_OK) return rc;
    MNF_REQUIRE(counts || n == 0, "voxel_walk_count: counts is null");
    MNF_REQUIRE(aligned8(counts), "voxel_walk_count: counts must be 8-byte aligned");
    if (n == 0) return MNF_OK;
    hipStream_t s = as_stream(stream);
    ProfScope prof("voxel_walk_count", s);
    hipLaunchKernelGGL(walk_count_kernel, dim3(blocks_for(n)), dim3(256), 0, s, start, end, current_voxel, end_voxel, n, voxel_size, (long long)max_steps,
                       reinterpret_cast<long long *>(counts), reinterpret_cast<unsigned long long *>(info));
    return launch_status("walk_count_kernel");
}

extern "C" int mnf_voxel_walk_fill(const double *start, const double *end, const int32_t *current_voxel, const int32_t *end_voxel, int64_t n, double voxel_size,
                                   int64_t max_steps, const int64_t *offsets, int64_t total, int32_t *voxels, int64_t *info, mnf_stream_t stream) {
    const int rc = walk_arguments("voxel_walk_fill", start, end, current_voxel, end_voxel, n, voxel_size, max_steps, info);
    if (rc != MNF_OK) return rc;
    MNF_REQUIRE(total >= 0 && total < ((int64_t)1 << 40), "voxel_walk_fill: total outside [0, 2^40) (%lld)", (long long)total);
    MNF_REQUIRE(offsets || n == 0, "voxel_walk_fill: offsets is null");
    MNF_REQUIRE(aligned8(offsets), "voxel_walk_fill: offsets must be 8-byte aligned");
    MNF_REQUIRE(voxels || total == 0, "voxel_walk_fill: voxels is null");
    if (n == 0) return MNF_OK;
    hipStream_t s = as_stream(stream);
    ProfScope prof("voxel_walk_fill", s);
    hipLaunchKernelGGL(walk_fill_kernel, dim3(blocks_for(n)), dim3(256), 0, s, start, end, current_voxel, end_voxel, n, voxel_size, (long long)max_steps, offsets,
                       total, voxels, reinterpret_cast<unsigned long long *>(info));
    return launch_status("walk_fill_kernel");
}

extern "C" int mnf_voxel_walk_hits(const double *start, const double *end, const int32_t *current_voxel, const int32_t *end_voxel, int64_t n, double voxel_size,
                                   int64_t max_steps, const uint8_t *binaries, int32_t n_members, int32_t X, int32_t Y, int32_t Z, int32_t *hits, int64_t *info,
                                   mnf_stream_t stream) {
    const int rc = walk_arguments("voxel_walk_hits", start, end, current_voxel, end_voxel, n, voxel_size, max_steps, info);
    if (rc != MNF_OK) return rc;
    BitGrid grid;
    MNF_REQUIRE(X > 0 && Y > 0 && Z > 0 && n_members > 0, "voxel_walk_hits: sizes must be positive (got %d members of %d x %d x %d)", n_members, X, Y, Z);
    MNF_REQUIRE(field_geometry_ok(n_members, X, Y, Z, &grid), "voxel_walk_hits: %d members of %d x %d x %d are outside the limits of a clearance field", n_members, X,
                Y, Z);
    MNF_REQUIRE(binaries, "voxel_walk_hits: binaries is null");
    MNF_REQUIRE(hits || n == 0, "voxel_walk_hits: hits is null");
    if (n == 0) return MNF_OK;
    hipStream_t s = as_stream(stream);
    ProfScope prof("voxel_walk_hits", s);
    hipLaunchKernelGGL(walk_hits_kernel, dim3(blocks_for(n)), dim3(256), 0, s, start, end, current_voxel, end_voxel, n, voxel_size, (long long)max_steps, binaries,
                       n_members, X, Y, Z, hits, reinterpret_cast<unsigned long long *>(info));
    return launch_status("walk_hits_kernel");
}
