// The exploration map on the device (gfx950): which voxels have been seen free, which seen occupied and which are still unknown, the top-down
// view of that, its frontier cells, their clusters and the nearest goal per cluster.
//   mnf_explore_map_insert             <- scripts/eval/frontier_baseline.py:170 (occ_grid.insert_depth_image: every pixel ray-cast through the grid)
//   mnf_explore_map_topdown            <- frontier_baseline.py:188 (get_occupancy_grid: 0 free, -1 unknown)
//   mnf_explore_map_frontiers          <- frontier_baseline.py:52-67 (find_frontiers, its inner-loop-only `break` included)
//   mnf_explore_map_frontier_clusters  <- frontier_baseline.py:191-214 (DBSCAN(eps=1, min_samples=3), the member nearest to the current pose)
//
// The map: uint32 bits[2][wpp], the bit grid of map_dev.h with two planes: plane 0 = "a ray passed through", plane 1 = "a ray ended here".
//
// Insert: one lane per pixel walks its voxels from the origin's to the end point's, exactly n_x + n_y + n_z steps (include/mi355nerf.h has the
// definition).  Built with -ffp-contract=off: every float expression is one separately rounded operation, as numpy evaluates it.  Only the
// resulting bits are specified, which leaves two freedoms the kernel uses: a lane stops once its ray has left the box for good (the path is
// monotone per axis), and it gathers the bits of consecutive steps that fall into one word (z runs fastest) into one test and one OR.
//
// Traffic.  Insert: 12 + 12 + 4 (+ 4) bytes per pixel read once; per word run of a walk one 4-byte load and, only where a bit of the run is still
// clear, one 32-bit atomic OR.  Neighbouring pixels walk nearly the same voxels, so most loads are L2 hits and most runs find their bits set.
// Read-outs: count and top-down read the two planes once; frontiers reads the [X][Z] byte map nine times (L1 / L2 hits) in one workgroup, in
// row-major order, which is what orders its output; the clusters are O(X Z + frontier cells).
#include "map_dev.h"
#include "workspace.h"

namespace mnf {
namespace {

constexpr float kMaxIndex = 16777216.0f;      // 2^24: below it a floored float converts to int exactly
constexpr int kMaxOffsets = 32;               // offsets with dx^2 + dz^2 <= 8, the centre excluded: 24

// ---------------------------------------------------------------------------------------------------------------- insert
// a plain load first, the atomic only where a bit of `m` is clear; a stale "clear" only repeats the OR.  (Joining the ORs of a wave's lanes into one per
// word was measured: 27 % faster into a cleared map, 22 % slower into a carved one, which is where a run inserts at every step but its first;
// profiles/exploration_map_wave_dedupe.txt.)
__device__ __forceinline__ void or_bits(unsigned int *word, unsigned int m, int &ors) {
    if ((*word & m) != m) { atomicOr(word, m); ++ors; }
}

__global__ void __launch_bounds__(256) explore_insert_kernel(
    const float *__restrict__ origins, const float *__restrict__ viewdirs, const float *__restrict__ depth, const float *__restrict__ acc, int64_t N,
    float gx, float gy, float gz, float vs, float inv, BitGrid g, float min_depth, float min_acc, float max_range, unsigned int *bits,
    unsigned long long *stats) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int steps = 0, ors = 0;
    do {                                                             // one pass; `break` skips the pixel
        if (i >= N) break;
        const float dep = depth[i];
        if (dep != dep || dep <= min_depth) break;
        if (acc && acc[i] < min_acc) break;
        const float o0 = origins[3 * i], o1 = origins[3 * i + 1], o2 = origins[3 * i + 2];
        const float d0 = viewdirs[3 * i], d1 = viewdirs[3 * i + 1], d2 = viewdirs[3 * i + 2];
        if (!(o0 - o0 == 0.0f && o1 - o1 == 0.0f && o2 - o2 == 0.0f && d0 - d0 == 0.0f && d1 - d1 == 0.0f && d2 - d2 == 0.0f)) break;
        const bool hit = dep - dep == 0.0f && dep <= max_range;
        const float t = hit ? dep : max_range;
        // per axis: first and last voxel, steps to take, their sign, the ray parameter of the next face and its increment per voxel
        int v0, v1, v2, n0, n1, n2, s0, s1, s2;
        float tm0, tm1, tm2, td0, td1, td2;
        bool ok = true;
#define MNF_AXIS(o, d, gm, v, n, s, tm, td)                                                        \
        {                                                                                          \
            const float fa = floorf((o - gm) * inv);                                               \
            const float step = t * d;                                                              \
            const float p = o + step;                                                              \
            const float fb = floorf((p - gm) * inv);                                               \
            ok = ok && fabsf(fa) < kMaxIndex && fabsf(fb) < kMaxIndex;             /* a NaN fails */ \
            v = ok ? (int)fa : 0;                                                                  \
            const int diff = ok ? (int)fb - v : 0;                                                 \
            n = diff < 0 ? -diff : diff;                                                           \
            s = (diff > 0) - (diff < 0);                                                           \
            tm = 0.0f; td = 0.0f;                                                                  \
            if (n > 0) {                                                             /* d != 0 */  \
                const float edge = (float)(v + (s > 0 ? 1 : 0)) * vs;                              \
                tm = ((gm + edge) - o) / d;                                                        \
                td = vs / fabsf(d);                                                                \
            }                                                                                      \
        }
        MNF_AXIS(o0, d0, gx, v0, n0, s0, tm0, td0)
        MNF_AXIS(o1, d1, gy, v1, n1, s1, tm1, td1)
        MNF_AXIS(o2, d2, gz, v2, n2, s2, tm2, td2)
#undef MNF_AXIS
        if (!ok) break;
        int rem = n0 + n1 + n2;                                      // <= 3 * 2^25
        int64_t cw = -1;                                             // the free-plane word the walk is gathering bits for, and those bits
        unsigned int cm = 0;
        for (;;) {
            // left the box on the side the axis moves to (or stands outside on an axis that does not move): nothing more to write
            if ((s0 >= 0 && v0 >= g.X) || (s0 <= 0 && v0 < 0) || (s1 >= 0 && v1 >= g.Y) || (s1 <= 0 && v1 < 0) || (s2 >= 0 && v2 >= g.Z) ||
                (s2 <= 0 && v2 < 0))
                break;
            const bool inside = (unsigned)v0 < (unsigned)g.X && (unsigned)v1 < (unsigned)g.Y && (unsigned)v2 < (unsigned)g.Z;
            const bool last = rem == 0;
            if (inside) {
                const int64_t lin = ((int64_t)v0 * g.Y + v1) * g.Z + v2;            // < n_vox: the word is inside its plane
                const int64_t w = lin >> 5;
                const unsigned int bit = 1u << (int)(lin & 31);
                if (last && hit) {
                    or_bits(bits + g.wpp + w, bit, ors);
                } else {
                    if (w != cw) {
                        if (cw >= 0) or_bits(bits + cw, cm, ors);
                        cw = w;
                        cm = 0;
                    }
                    cm |= bit;
                }
            }
            if (last) break;
            // the first axis in x, y, z order with steps left; a later one replaces it only with a strictly smaller tm
            int best = -1;
            float bt = 0.0f;
            if (n0 > 0) { best = 0; bt = tm0; }
            if (n1 > 0 && (best < 0 || tm1 < bt)) { best = 1; bt = tm1; }
            if (n2 > 0 && (best < 0 || tm2 < bt)) { best = 2; }
            if (best == 0) { v0 += s0; --n0; tm0 = tm0 + td0; }
            else if (best == 1) { v1 += s1; --n1; tm1 = tm1 + td1; }
            else { v2 += s2; --n2; tm2 = tm2 + td2; }
            --rem;
            ++steps;
        }
        if (cw >= 0) or_bits(bits + cw, cm, ors);
    } while (false);
    if (stats) {                                                     // (uniform) the measurement's counters: voxel steps walked, ORs issued
        unsigned long long a = (unsigned long long)steps, b = (unsigned long long)ors;
        wave_sum_each(a, b);
        if ((threadIdx.x & 63) == 0) { atomicAdd(stats, a); atomicAdd(stats + 1, b); }
    }
}

// ---------------------------------------------------------------------------------------------------------------- count
// counts[] is zeroed before the launch; integer atomics: exact, whatever the order
__global__ void __launch_bounds__(256) explore_count_kernel(const unsigned int *__restrict__ bits, BitGrid g, int64_t *__restrict__ counts) {
    __shared__ int64_t red[4][3];
    const int tid = threadIdx.x;
    const int64_t words = (g.n_vox + 31) >> 5;
    int64_t fr = 0, oc = 0, un = 0;
    for (int64_t w = (int64_t)blockIdx.x * 256 + tid; w < words; w += (int64_t)gridDim.x * 256) {
        const unsigned int valid = valid_bits(w, g.n_vox), p0 = bits[w], p1 = bits[g.wpp + w];
        const int o = __popc(p1 & valid), f = __popc(p0 & ~p1 & valid);
        oc += o; fr += f; un += __popc(valid) - o - f;
    }
    wave_sum_each(fr, oc, un);
    if ((tid & 63) == 0) { red[tid >> 6][0] = fr; red[tid >> 6][1] = oc; red[tid >> 6][2] = un; }
    __syncthreads();
    if (tid < 3) {
        const int64_t s = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
        if (s) atomicAdd(reinterpret_cast<unsigned long long *>(counts + tid), (unsigned long long)s);
    }
}

// ---------------------------------------------------------------------------------------------------------------- top-down
// one lane per cell (x, z); neighbouring lanes read neighbouring bits
__global__ void __launch_bounds__(256) explore_topdown_kernel(const unsigned int *__restrict__ bits, BitGrid g, int y_lo, int y_hi, int8_t *__restrict__ map) {
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= (int64_t)g.X * g.Z) return;
    const int64_t x = c / g.Z, z = c - x * g.Z;
    bool occ = false, fre = false;
    for (int y = y_lo; y < y_hi && !occ; ++y) {
        const int64_t lin = (x * g.Y + y) * g.Z + z;
        const int64_t w = lin >> 5;
        const int bit = (int)(lin & 31);
        occ = (bits[g.wpp + w] >> bit) & 1u;
        fre = fre || ((bits[w] >> bit) & 1u);
    }
    map[c] = occ ? 1 : fre ? 0 : -1;
}

// ---------------------------------------------------------------------------------------------------------------- frontiers
constexpr int kFrontierThreads = 1024;

// ONE workgroup walks the cells in row-major order, 1024 at a time, and appends the frontier cells of each batch behind those of the batches
// before it: the output is ordered without a workspace.  At most X Z cells; a map of 500 x 500 is 245 batches.
__global__ void __launch_bounds__(kFrontierThreads) explore_frontiers_kernel(const int8_t *__restrict__ map, int X, int Z, int64_t cap, int *__restrict__ cells,
                                                                            int *__restrict__ mult, int64_t *__restrict__ info) {
    const int tid = threadIdx.x;
    const int64_t total = (int64_t)X * Z;
    int64_t base = 0;
    for (int64_t c0 = 0; c0 < total; c0 += kFrontierThreads) {
        const int64_t c = c0 + tid;
        int m = 0, x = 0, z = 0;
        if (c < total && map[c] == 0) {
            x = (int)(c / Z);
            z = (int)(c - (int64_t)x * Z);
            for (int dx = -1; dx <= 1; ++dx) {                       // once per dx whose column holds an unknown neighbour: the reference's list
                const int nx = x + dx;
                if (nx < 0 || nx >= X) continue;
                bool any = false;
                for (int dz = -1; dz <= 1; ++dz) {
                    const int nz = z + dz;
                    if (nz >= 0 && nz < Z && map[(int64_t)nx * Z + nz] == -1) any = true;
                }
                m += any ? 1 : 0;
            }
        }
        int all;
        const int64_t r = base + block_rank<kFrontierThreads>(m > 0, &all);
        if (m > 0 && r < cap) { cells[2 * r] = x; cells[2 * r + 1] = z; mult[r] = m; }
        base += all;
    }
    if (tid == 0) { info[0] = base; info[1] = base > cap ? 1 : 0; }
}

// ---------------------------------------------------------------------------------------------------------------- frontier clusters
struct Offsets { int n; signed char d[kMaxOffsets][2]; };

// the caller's workspace; every array starts 8-byte aligned
struct ClusterWs {
    int64_t *flag, *row, *scan, *totals;          // totals[0]: clusters
    unsigned long long *best;                     // per cluster: the smallest squared distance, as the bits of a non-negative double
    int *index, *parent, *core, *goal;            // index[X Z]: a cell's position in the list or -1
    int64_t bytes;
};

inline ClusterWs carve(void *base, int64_t cells, int64_t mf, int64_t mc) {
    Carver c(base, 8);
    ClusterWs w;
    w.flag = c.take<int64_t>(mf);
    w.row = c.take<int64_t>(mf);
    w.scan = (int64_t *)c.take(scan_bytes(mf));
    w.totals = c.take<int64_t>(1);
    w.best = c.take<unsigned long long>(mc);
    w.index = c.take<int>(cells);
    w.parent = c.take<int>(mf);
    w.core = c.take<int>(mf);
    w.goal = c.take<int>(mc);
    w.bytes = c.bytes();
    return w;
}

__device__ __forceinline__ int64_t listed(const int64_t *__restrict__ finfo, int64_t mf) { return finfo[0] < mf ? finfo[0] : mf; }

__global__ void __launch_bounds__(256) fc_clear_kernel(int64_t cells, int64_t mc, int *__restrict__ index, unsigned long long *__restrict__ best,
                                                      int *__restrict__ goal, int *__restrict__ sizes) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < cells) index[i] = -1;
    if (i < mc) { best[i] = ~0ull; goal[i] = 0x7fffffff; sizes[i] = 0; }
}

__global__ void __launch_bounds__(256) fc_index_kernel(const int *__restrict__ cells, const int64_t *__restrict__ finfo, int64_t mf, int X, int Z,
                                                      int *__restrict__ index, int *__restrict__ parent) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= listed(finfo, mf)) return;
    const int x = cells[2 * i], z = cells[2 * i + 1];
    parent[i] = (int)i;
    if (x >= 0 && x < X && z >= 0 && z < Z) index[(int64_t)x * Z + z] = (int)i;       // a cell outside the map links to nothing
}

// the list position of the cell at (x + dx, z + dz), or -1
__device__ __forceinline__ int neighbour(const int *__restrict__ index, int X, int Z, int x, int z, int dx, int dz) {
    const int nx = x + dx, nz = z + dz;
    if (nx < 0 || nx >= X || nz < 0 || nz >= Z) return -1;
    return index[(int64_t)nx * Z + nz];
}

__global__ void __launch_bounds__(256) fc_core_kernel(const int *__restrict__ cells, const int *__restrict__ mult, const int64_t *__restrict__ finfo, int64_t mf,
                                                     int X, int Z, Offsets offs, int min_samples, int weighted, const int *__restrict__ index,
                                                     int *__restrict__ core) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= listed(finfo, mf)) return;
    const int x = cells[2 * i], z = cells[2 * i + 1];
    int64_t sum = weighted ? mult[i] : 1;
    for (int k = 0; k < offs.n; ++k) {
        const int j = neighbour(index, X, Z, x, z, offs.d[k][0], offs.d[k][1]);
        if (j >= 0) sum += weighted ? mult[j] : 1;
    }
    core[i] = sum >= min_samples ? 1 : 0;
}

// the union-find over the list positions of the core cells: map_dev.h
__global__ void __launch_bounds__(256) fc_link_kernel(const int *__restrict__ cells, const int64_t *__restrict__ finfo, int64_t mf, int X, int Z, Offsets offs,
                                                     const int *__restrict__ index, const int *__restrict__ core, int *parent) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= listed(finfo, mf) || !core[i]) return;
    const int x = cells[2 * i], z = cells[2 * i + 1];
    for (int k = 0; k < offs.n; ++k) {
        const int j = neighbour(index, X, Z, x, z, offs.d[k][0], offs.d[k][1]);
        if (j > (int)i && core[j]) unite(parent, (int)i, j);         // each pair once, from its smaller member
    }
}

// 1 at every core cell that is its component's root, over the whole capacity (the scan's length is the capacity)
__global__ void __launch_bounds__(256) fc_flag_kernel(const int *__restrict__ parent, const int *__restrict__ core, const int64_t *__restrict__ finfo, int64_t mf,
                                                     int64_t *__restrict__ flag) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= mf) return;
    flag[i] = (i < listed(finfo, mf) && core[i] && parent[i] == (int)i) ? 1 : 0;
}

// labels, member counts and the smallest squared distance per cluster (the link launch is over: parent[] is read-only here)
__global__ void __launch_bounds__(256) fc_label_kernel(const int *__restrict__ cells, const int64_t *__restrict__ finfo, int64_t mf, int X, int Z, Offsets offs,
                                                      const int *__restrict__ index, const int *__restrict__ core, const int *__restrict__ parent,
                                                      const int64_t *__restrict__ row, double cur_x, double cur_z, int64_t mc, int *__restrict__ labels,
                                                      int *__restrict__ sizes, unsigned long long *__restrict__ best) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= listed(finfo, mf)) return;
    const int x = cells[2 * i], z = cells[2 * i + 1];
    int64_t label = -1;
    if (core[i]) {
        label = row[settled_root(parent, (int)i)];
    } else {
        for (int k = 0; k < offs.n; ++k) {                           // the smallest label among the core neighbours
            const int j = neighbour(index, X, Z, x, z, offs.d[k][0], offs.d[k][1]);
            if (j < 0 || !core[j]) continue;
            const int64_t l = row[settled_root(parent, j)];
            if (label < 0 || l < label) label = l;
        }
    }
    labels[i] = (int)label;
    if (label < 0 || label >= mc) return;
    atomicAdd(sizes + label, 1);
    const double dx = (double)x - cur_x, dz = (double)z - cur_z;
    const double d2 = dx * dx + dz * dz;                             // >= 0 and finite: ordered as its bit pattern
    atomicMin(best + label, (unsigned long long)__double_as_longlong(d2));
}

// of the members at the smallest distance, the first in the list (the lowest row-major cell)
__global__ void __launch_bounds__(256) fc_pick_kernel(const int *__restrict__ cells, const int64_t *__restrict__ finfo, int64_t mf, const int *__restrict__ labels,
                                                     const unsigned long long *__restrict__ best, double cur_x, double cur_z, int64_t mc, int *__restrict__ goal) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= listed(finfo, mf)) return;
    const int label = labels[i];
    if (label < 0 || label >= mc) return;
    const double dx = (double)cells[2 * i] - cur_x, dz = (double)cells[2 * i + 1] - cur_z;
    const double d2 = dx * dx + dz * dz;
    if ((unsigned long long)__double_as_longlong(d2) == best[label]) atomicMin(goal + label, (int)i);
}

__global__ void __launch_bounds__(256) fc_finish_kernel(const int *__restrict__ cells, const int64_t *__restrict__ totals, const int *__restrict__ goal, int64_t mc,
                                                       int *__restrict__ goals, int64_t *__restrict__ info) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t found = totals[0];
    if (i == 0) { info[0] = found; info[1] = found > mc ? 1 : 0; }
    if (i >= found || i >= mc) return;
    const int gi = goal[i];                                          // every cluster has a core member, so a goal
    goals[2 * i] = cells[2 * gi];
    goals[2 * i + 1] = cells[2 * gi + 1];
}

}  // namespace
}  // namespace mnf

using namespace mnf;

extern "C" int64_t mnf_explore_map_bytes(int32_t res_x, int32_t res_y, int32_t res_z) {
    BitGrid g;
    if (!make_bit_grid(2, res_x, res_y, res_z, &g)) return 0;
    return g.wpp * 2 * (int64_t)sizeof(uint32_t);
}

extern "C" int mnf_explore_map_insert(uint32_t *bits, int32_t res_x, int32_t res_y, int32_t res_z, const float *grid_min_host, float voxel_size,
                                      float max_range, const float *origins, const float *viewdirs, const float *depth, const float *acc,
                                      int64_t n_rays, float min_depth, float min_acc, int64_t *stats, mnf_stream_t stream) {
    BitGrid g;
    MNF_REQUIRE(res_x > 0 && res_y > 0 && res_z > 0, "explore_map_insert: resolution must be positive (got %d x %d x %d)", res_x, res_y, res_z);
    MNF_REQUIRE(make_bit_grid(2, res_x, res_y, res_z, &g), "explore_map_insert: resolution %d x %d x %d is more than the map indexes", res_x, res_y, res_z);
    MNF_REQUIRE(voxel_size > 0.0f && voxel_size - voxel_size == 0.0f, "explore_map_insert: voxel_size must be positive and finite (got %g)", (double)voxel_size);
    MNF_REQUIRE(max_range > 0.0f && max_range - max_range == 0.0f, "explore_map_insert: max_range must be positive and finite (got %g)", (double)max_range);
    MNF_REQUIRE(max_range / voxel_size <= 1048576.0f, "explore_map_insert: max_range / voxel_size is more than 2^20 voxels (got %g)",
                (double)(max_range / voxel_size));
    MNF_REQUIRE(n_rays >= 0, "explore_map_insert: n_rays is negative (%lld)", (long long)n_rays);
    MNF_REQUIRE(n_rays <= (int64_t)0x7fffffff * 256, "explore_map_insert: n_rays is more than one launch holds (%lld)", (long long)n_rays);
    MNF_REQUIRE(grid_min_host, "explore_map_insert: grid_min is null");
    MNF_REQUIRE(min_depth == min_depth && min_acc == min_acc, "explore_map_insert: min_depth or min_acc is NaN");
    MNF_REQUIRE(bits || n_rays == 0, "explore_map_insert: bits is null");
    MNF_REQUIRE(origins || n_rays == 0, "explore_map_insert: origins is null");
    MNF_REQUIRE(viewdirs || n_rays == 0, "explore_map_insert: viewdirs is null");
    MNF_REQUIRE(depth || n_rays == 0, "explore_map_insert: depth is null");
    MNF_REQUIRE(aligned8(bits), "explore_map_insert: bits must be 8-byte aligned");
    MNF_REQUIRE(aligned8(stats), "explore_map_insert: stats must be 8-byte aligned");
    if (n_rays == 0) return MNF_OK;
    const float inv = 1.0f / voxel_size;
    hipStream_t s = as_stream(stream);
    ProfScope prof("explore_map_insert", s);
    hipLaunchKernelGGL(explore_insert_kernel, dim3(blocks_for(n_rays)), dim3(256), 0, s, origins, viewdirs, depth, acc, n_rays, grid_min_host[0],
                       grid_min_host[1], grid_min_host[2], voxel_size, inv, g, min_depth, min_acc, max_range, bits,
                       reinterpret_cast<unsigned long long *>(stats));
    return launch_status("explore_insert_kernel");
}

extern "C" int mnf_explore_map_count(const uint32_t *bits, int32_t res_x, int32_t res_y, int32_t res_z, int64_t *counts, mnf_stream_t stream) {
    BitGrid g;
    MNF_REQUIRE(make_bit_grid(2, res_x, res_y, res_z, &g), "explore_map_count: bad geometry (resolution %d x %d x %d)", res_x, res_y, res_z);
    MNF_REQUIRE(bits, "explore_map_count: bits is null");
    MNF_REQUIRE(counts, "explore_map_count: counts is null");
    hipStream_t s = as_stream(stream);
    ProfScope prof("explore_map_count", s);
    MNF_HIP(hipMemsetAsync(counts, 0, 3 * sizeof(int64_t), s));
    const int64_t words = (g.n_vox + 31) >> 5;
    const unsigned nb = blocks_for(words) < 1024u ? blocks_for(words) : 1024u;
    hipLaunchKernelGGL(explore_count_kernel, dim3(nb), dim3(256), 0, s, bits, g, counts);
    return launch_status("explore_count_kernel");
}

extern "C" int mnf_explore_map_topdown(const uint32_t *bits, int32_t res_x, int32_t res_y, int32_t res_z, int32_t y_lo, int32_t y_hi, int8_t *map,
                                       mnf_stream_t stream) {
    BitGrid g;
    MNF_REQUIRE(make_bit_grid(2, res_x, res_y, res_z, &g), "explore_map_topdown: bad geometry (resolution %d x %d x %d)", res_x, res_y, res_z);
    MNF_REQUIRE(y_lo >= 0 && y_lo <= y_hi && y_hi <= res_y, "explore_map_topdown: layers [y_lo, y_hi) = [%d, %d) outside [0, %d]", y_lo, y_hi, res_y);
    MNF_REQUIRE(bits, "explore_map_topdown: bits is null");
    MNF_REQUIRE(map, "explore_map_topdown: map is null");
    hipStream_t s = as_stream(stream);
    ProfScope prof("explore_map_topdown", s);
    hipLaunchKernelGGL(explore_topdown_kernel, dim3(blocks_for((int64_t)res_x * res_z)), dim3(256), 0, s, bits, g, y_lo, y_hi, map);
    return launch_status("explore_topdown_kernel");
}

extern "C" int mnf_explore_map_frontiers(const int8_t *map, int32_t res_x, int32_t res_z, int64_t max_frontiers, int32_t *cells, int32_t *mult,
                                         int64_t *info, mnf_stream_t stream) {
    MNF_REQUIRE(res_x > 0 && res_z > 0 && res_x <= kMaxAxis && res_z <= kMaxAxis && (int64_t)res_x * res_z <= 0x7fffffff,
                "explore_map_frontiers: bad geometry (resolution %d x %d)", res_x, res_z);
    MNF_REQUIRE(max_frontiers >= 0 && max_frontiers <= 0x7fffffff, "explore_map_frontiers: max_frontiers outside [0, 2^31) (got %lld)", (long long)max_frontiers);
    MNF_REQUIRE(map, "explore_map_frontiers: map is null");
    MNF_REQUIRE(cells || max_frontiers == 0, "explore_map_frontiers: cells is null");
    MNF_REQUIRE(mult || max_frontiers == 0, "explore_map_frontiers: mult is null");
    MNF_REQUIRE(info, "explore_map_frontiers: info is null");
    hipStream_t s = as_stream(stream);
    ProfScope prof("explore_map_frontiers", s);
    hipLaunchKernelGGL(explore_frontiers_kernel, dim3(1), dim3(kFrontierThreads), 0, s, map, res_x, res_z, max_frontiers, cells, mult, info);
    return launch_status("explore_frontiers_kernel");
}

extern "C" int64_t mnf_explore_map_frontier_clusters_workspace_bytes(int32_t res_x, int32_t res_z, int64_t max_frontiers, int64_t max_clusters) {
    if (res_x <= 0 || res_z <= 0 || res_x > kMaxAxis || res_z > kMaxAxis || (int64_t)res_x * res_z > 0x7fffffff) return 0;
    if (max_frontiers < 0 || max_frontiers > 0x7fffffff || max_clusters < 0 || max_clusters > 0x7fffffff) return 0;
    return carve(nullptr, (int64_t)res_x * res_z, max_frontiers, max_clusters).bytes;
}

extern "C" int mnf_explore_map_frontier_clusters(const int32_t *cells, const int32_t *mult, const int64_t *frontier_info, int64_t max_frontiers,
                                                 int32_t res_x, int32_t res_z, int32_t eps2, int32_t min_samples, int32_t weighted, double current_x,
                                                 double current_z, int64_t max_clusters, int32_t *labels, int32_t *goals, int32_t *sizes,
                                                 int64_t *info, void *workspace, int64_t workspace_bytes, mnf_stream_t stream) {
    MNF_REQUIRE(res_x > 0 && res_z > 0 && res_x <= kMaxAxis && res_z <= kMaxAxis && (int64_t)res_x * res_z <= 0x7fffffff,
                "explore_map_frontier_clusters: bad geometry (resolution %d x %d)", res_x, res_z);
    MNF_REQUIRE(eps2 >= 1 && eps2 <= 8, "explore_map_frontier_clusters: eps2 must lie in 1 .. 8 (got %d)", eps2);
    MNF_REQUIRE(min_samples >= 1, "explore_map_frontier_clusters: min_samples must be at least 1 (got %d)", min_samples);
    MNF_REQUIRE(max_frontiers >= 0 && max_frontiers <= 0x7fffffff, "explore_map_frontier_clusters: max_frontiers outside [0, 2^31) (got %lld)",
                (long long)max_frontiers);
    MNF_REQUIRE(max_clusters >= 0 && max_clusters <= 0x7fffffff, "explore_map_frontier_clusters: max_clusters outside [0, 2^31) (got %lld)",
                (long long)max_clusters);
    MNF_REQUIRE(finite_d(current_x) && finite_d(current_z), "explore_map_frontier_clusters: current is not finite");
    MNF_REQUIRE(cells || max_frontiers == 0, "explore_map_frontier_clusters: cells is null");
    MNF_REQUIRE(mult || max_frontiers == 0, "explore_map_frontier_clusters: mult is null");
    MNF_REQUIRE(frontier_info, "explore_map_frontier_clusters: frontier_info is null");
    MNF_REQUIRE(labels || max_frontiers == 0, "explore_map_frontier_clusters: labels is null");
    MNF_REQUIRE(goals || max_clusters == 0, "explore_map_frontier_clusters: goals is null");
    MNF_REQUIRE(sizes || max_clusters == 0, "explore_map_frontier_clusters: sizes is null");
    MNF_REQUIRE(info, "explore_map_frontier_clusters: info is null");
    MNF_REQUIRE(workspace, "explore_map_frontier_clusters: workspace is null");
    MNF_REQUIRE(aligned8(workspace), "explore_map_frontier_clusters: workspace must be 8-byte aligned");
    const int64_t n_cells = (int64_t)res_x * res_z, mf = max_frontiers, mc = max_clusters;
    const ClusterWs w = carve(workspace, n_cells, mf, mc);
    MNF_REQUIRE(workspace_bytes >= w.bytes, "explore_map_frontier_clusters: workspace too small (%lld < %lld bytes)", (long long)workspace_bytes,
                (long long)w.bytes);
    Offsets offs;
    offs.n = 0;
    for (int dx = -2; dx <= 2; ++dx)
        for (int dz = -2; dz <= 2; ++dz) {
            if ((dx == 0 && dz == 0) || dx * dx + dz * dz > eps2) continue;
            offs.d[offs.n][0] = (signed char)dx; offs.d[offs.n][1] = (signed char)dz;
            ++offs.n;
        }
    hipStream_t s = as_stream(stream);
    ProfScope prof("explore_map_frontier_clusters", s);
    hipLaunchKernelGGL(fc_clear_kernel, dim3(blocks_for(n_cells > mc ? n_cells : mc)), dim3(256), 0, s, n_cells, mc, w.index, w.best, w.goal, sizes);
    hipLaunchKernelGGL(fc_index_kernel, dim3(blocks_for(mf)), dim3(256), 0, s, cells, frontier_info, mf, res_x, res_z, w.index, w.parent);
    hipLaunchKernelGGL(fc_core_kernel, dim3(blocks_for(mf)), dim3(256), 0, s, cells, mult, frontier_info, mf, res_x, res_z, offs, min_samples, weighted,
                       w.index, w.core);
    hipLaunchKernelGGL(fc_link_kernel, dim3(blocks_for(mf)), dim3(256), 0, s, cells, frontier_info, mf, res_x, res_z, offs, w.index, w.core, w.parent);
    hipLaunchKernelGGL(fc_flag_kernel, dim3(blocks_for(mf)), dim3(256), 0, s, w.parent, w.core, frontier_info, mf, w.flag);
    int rc = launch_status("fc_flag_kernel");
    if (rc) return rc;
    rc = mnf_exclusive_scan_i64(w.flag, mf, w.row, w.totals, w.scan, scan_bytes(mf), stream);
    if (rc) return rc;
    hipLaunchKernelGGL(fc_label_kernel, dim3(blocks_for(mf)), dim3(256), 0, s, cells, frontier_info, mf, res_x, res_z, offs, w.index, w.core, w.parent, w.row,
                       current_x, current_z, mc, labels, sizes, w.best);
    hipLaunchKernelGGL(fc_pick_kernel, dim3(blocks_for(mf)), dim3(256), 0, s, cells, frontier_info, mf, labels, w.best, current_x, current_z, mc, w.goal);
    hipLaunchKernelGGL(fc_finish_kernel, dim3(blocks_for(mc)), dim3(256), 0, s, cells, w.totals, w.goal, mc, goals, info);
    return launch_status("fc_finish_kernel");
}
