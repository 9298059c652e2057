// The semantic object map on the device (gfx950): one bit plane per class over a voxel grid, its clusters and their match to a list of
// ground-truth objects.
//   mnf_object_map_insert    <- scripts/eval/eval_pipeline_offline.py:119-138 (per view and per class: a NaN-masked copy of the depth image
//                               pushed through VoxelGrid.insert_depth_image)
//   mnf_object_map_clusters  <- eval_pipeline_offline.py:26-42 (get_pointcloud, DBSCAN(eps=0.2, min_samples=1), the mean per label)
//   mnf_object_map_match     <- eval_pipeline_offline.py:45-70 (greedy nearest unmatched ground-truth object per cluster)
//
// The map: uint32 bits[C][wpp], the bit grid of map_dev.h with one plane per class.
//
// Linkage is defined on integer voxel offsets (dx^2 + dy^2 + dz^2 <= link_r2), so with min_samples = 1 the clusters are the connected
// components of that graph: the union-find of map_dev.h over the RANKS of the set voxels (rank = position in class-then-linear-index order,
// found in constant time as prefix[word] + popc(word & below)).  A component's root is then its smallest rank whatever the schedule, the
// per-cluster sums are integers, and the centroid is formed from them in float64: the same grid gives the same bytes.  Built with
// -ffp-contract=off: every float expression is one separately rounded operation, as numpy evaluates it.
//
// Traffic.  Insert: 12 + 12 + 4 (+ 4) bytes of rays, depth and acc and 4 C bytes of logits per pixel, read once (the logits through LDS:
// view_dev.h's stage_rows), one 4-byte bit test and, only where the bit is clear, one 32-bit atomic OR.  Clusters: the bit grid is read three
// times (popcount, enumerate, and as the neighbour test of the link pass: 16 word reads per set voxel at link_r2 = 4, L2 hits), the rest is
// O(set voxels).
#include "map_dev.h"
#include "view_dev.h"
#include "workspace.h"

namespace mnf {
namespace {

constexpr int kInsertMaxBlocks = 2048;
constexpr int kMaxOffsets = 64;               // forward half of the offsets with squared length <= 8: 58

// ---------------------------------------------------------------------------------------------------------------- insert
__global__ void __launch_bounds__(kViewThreads) object_map_insert_kernel(
    const float *__restrict__ origins, const float *__restrict__ viewdirs, const float *__restrict__ depth, const float *__restrict__ acc,
    const float *__restrict__ sem, const void *__restrict__ labels, int label_is_u8, int64_t N, int C, int tp, int64_t tiles,
    float gx, float gy, float gz, float inv, BitGrid g, int first_class, float min_depth, float max_depth, float min_acc,
    unsigned int *__restrict__ bits) {
    extern __shared__ float stage[];                                 // [tp][C | 1], logits only
    const int tid = threadIdx.x, nb = gridDim.x, b = blockIdx.x;
    const int Cs = C | 1;
    const int64_t t0 = tiles * b / nb, t1 = tiles * (b + 1) / nb;
    for (int64_t t = t0; t < t1; ++t) {
        const int64_t p0 = t * tp;
        const int np = (int)(N - p0 < tp ? N - p0 : tp);
        if (sem) {
            __syncthreads();                                         // the previous tile's rows are read
            stage_rows(stage, sem + p0 * C, np * C, C, Cs, tid);
            __syncthreads();
        }
        if (tid >= np) continue;
        const int64_t i = p0 + tid;
        int64_t cls;
        if (sem) {
            float best;
            cls = first_argmax(stage + tid * Cs, C, &best);
        } else {
            cls = label_is_u8 ? (int64_t)reinterpret_cast<const uint8_t *>(labels)[i] : reinterpret_cast<const int64_t *>(labels)[i];
        }
        if (cls < first_class || cls >= C) continue;
        const float dep = depth[i];
        if (!(dep - dep == 0.0f)) continue;                          // NaN, +-inf
        if (dep <= min_depth || dep > max_depth) continue;
        if (acc && acc[i] < min_acc) continue;
        const float gmin[3] = {gx, gy, gz};
        const int res[3] = {g.X, g.Y, g.Z};
        int v[3];
        bool inside = true;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float step = dep * viewdirs[3 * i + k];
            const float p = origins[3 * i + k] + step;
            const float rel = p - gmin[k];
            const float f = floorf(rel * inv);
            inside = inside && f >= 0.0f && f < (float)res[k];      // a NaN fails both
            v[k] = inside ? (int)f : 0;
        }
        if (!inside) continue;
        const int64_t lin = ((int64_t)v[0] * g.Y + v[1]) * g.Z + v[2];
        unsigned int *word = bits + cls * g.wpp + (lin >> 5);
        const unsigned int bit = 1u << (int)(lin & 31);
        if (!(*word & bit)) atomicOr(word, bit);                     // a stale "clear" only repeats the OR
    }
}

// ---------------------------------------------------------------------------------------------------------------- count
// one workgroup per class
__global__ void __launch_bounds__(256) object_map_count_kernel(const unsigned int *__restrict__ bits, BitGrid g, int64_t *__restrict__ counts) {
    __shared__ int64_t red[4];
    const int c = blockIdx.x, tid = threadIdx.x;
    const int64_t words = (g.n_vox + 31) >> 5;
    int64_t n = 0;
    for (int64_t w = tid; w < words; w += 256) n += __popc(bits[c * g.wpp + w] & valid_bits(w, g.n_vox));
    n = wave_sum(n);
    if ((tid & 63) == 0) red[tid >> 6] = n;
    __syncthreads();
    if (tid == 0) counts[c] = (red[0] + red[1]) + (red[2] + red[3]);
}

// ---------------------------------------------------------------------------------------------------------------- clusters
struct Offsets { int n; signed char d[kMaxOffsets][3]; };

// the caller's workspace; every array starts 8-byte aligned
struct ClusterWs {
    int64_t *wordcnt, *prefix, *scan, *totals;   // totals[0]: set voxels, totals[1]: clusters kept
    int64_t *vox, *flag, *row, *sums;
    int *parent, *root, *size;
    int64_t bytes;
};

inline ClusterWs carve(void *base, const BitGrid &g, int C, int64_t mv) {
    Carver c(base, 8);
    const int64_t nw = g.wpp * C;
    ClusterWs w;
    w.wordcnt = c.take<int64_t>(nw);
    w.prefix = c.take<int64_t>(nw);
    w.scan = (int64_t *)c.take(scan_bytes(nw > mv ? nw : mv));
    w.totals = c.take<int64_t>(2);
    w.vox = c.take<int64_t>(mv);
    w.flag = c.take<int64_t>(mv);
    w.row = c.take<int64_t>(mv);
    w.sums = c.take<int64_t>(mv * 4);                                // a row per kept cluster: there are no more clusters than voxels
    w.parent = c.take<int>(mv);
    w.root = c.take<int>(mv);
    w.size = c.take<int>(mv);
    w.bytes = c.bytes();
    return w;
}

__global__ void __launch_bounds__(256) popcount_words_kernel(const unsigned int *__restrict__ bits, BitGrid g, int64_t nw, int64_t *__restrict__ wordcnt) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nw) return;
    wordcnt[i] = __popc(bits[i] & valid_bits(i % g.wpp, g.n_vox));
}

// info, and the accumulators the later kernels add into
__global__ void __launch_bounds__(256) clusters_init_kernel(const int64_t *__restrict__ totals, int64_t mv, int64_t mc, int C, int64_t *__restrict__ sums,
                                                           int64_t *__restrict__ cluster_counts, int64_t *__restrict__ info) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t total = totals[0];
    if (i == 0) { info[0] = total; info[1] = 0; info[2] = total > mv ? 1 : 0; info[3] = 0; }
    if (total > mv) return;
    if (i < (mc < mv ? mc : mv) * 4) sums[i] = 0;
    if (i < C) cluster_counts[i] = 0;
}

// one lane per word: the set voxels in class-then-linear-index order
__global__ void __launch_bounds__(256) enumerate_kernel(const unsigned int *__restrict__ bits, BitGrid g, int64_t nw, const int64_t *__restrict__ prefix,
                                                       const int64_t *__restrict__ totals, int64_t mv, int64_t *__restrict__ vox, int *__restrict__ parent,
                                                       int *__restrict__ size, int64_t *__restrict__ voxel_ids) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nw || totals[0] > mv) return;
    const int64_t c = i / g.wpp, w = i - c * g.wpp;
    unsigned int m = bits[i] & valid_bits(w, g.n_vox);
    int64_t rank = prefix[i];
    while (m) {
        const int bit = __ffs((int)m) - 1;
        m &= m - 1;
        const int64_t id = c * g.n_vox + w * 32 + bit;
        vox[rank] = id;
        parent[rank] = (int)rank;
        size[rank] = 0;
        if (voxel_ids) voxel_ids[rank] = id;
        ++rank;
    }
}

// the union-find over the ranks: map_dev.h
__global__ void __launch_bounds__(256) link_kernel(const unsigned int *__restrict__ bits, BitGrid g, const int64_t *__restrict__ prefix,
                                                  const int64_t *__restrict__ totals, int64_t mv, const int64_t *__restrict__ vox, Offsets offs,
                                                  int *parent) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t total = totals[0];
    if (total > mv || i >= total) return;
    const int64_t id = vox[i];
    const int64_t c = id / g.n_vox, lin = id - c * g.n_vox;
    const int z = (int)(lin % g.Z), y = (int)((lin / g.Z) % g.Y), x = (int)(lin / ((int64_t)g.Z * g.Y));
    const unsigned int *plane = bits + c * g.wpp;                    // neighbours are looked up in the voxel's own plane only
    const int64_t *pre = prefix + c * g.wpp;
    for (int k = 0; k < offs.n; ++k) {
        const int nx = x + offs.d[k][0], ny = y + offs.d[k][1], nz = z + offs.d[k][2];
        if (nx < 0 || nx >= g.X || ny < 0 || ny >= g.Y || nz < 0 || nz >= g.Z) continue;     // in 3-D, never in linear index
        const int64_t nlin = ((int64_t)nx * g.Y + ny) * g.Z + nz;
        const int64_t w = nlin >> 5;
        const int bit = (int)(nlin & 31);
        const unsigned int m = plane[w];
        if (!((m >> bit) & 1u)) continue;
        const int64_t j = pre[w] + __popc(m & ((1u << bit) - 1u));
        unite(parent, (int)i, (int)j);
    }
}

// Sum of v over each run of equal keys among the 64 lanes, left in the run's first lane.  `run_end` is the last lane of the caller's run.
__device__ __forceinline__ int64_t run_sum(int64_t v, int lane, int run_end) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int64_t u = __shfl_down(v, off, 64);
        if (lane + off <= run_end) v += u;
    }
    return v;
}

// first and last lane of the run of equal keys that holds this lane (every lane of the wave calls it)
__device__ __forceinline__ void run_bounds(int64_t key, int lane, bool *head, int *run_end) {
    const int64_t prev = __shfl_up(key, 1, 64);
    *head = lane == 0 || prev != key;
    const unsigned long long heads = __ballot(*head);
    const unsigned long long after = lane == 63 ? 0ull : heads & ~((2ull << lane) - 1ull);
    *run_end = after ? __ffsll((long long)after) - 2 : 63;
}

// every voxel's root (the link launch is over: parent[] is read-only here) and every root's voxel count
__global__ void __launch_bounds__(256) roots_kernel(const int *__restrict__ parent, const int64_t *__restrict__ totals, int64_t mv,
                                                   int *__restrict__ root, int *__restrict__ size) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t total = totals[0];
    if (total > mv) return;                                          // (uniform)
    const bool live = i < total;
    int r = -1;
    if (live) {
        r = settled_root(parent, (int)i);
        root[i] = r;
    }
    const int lane = threadIdx.x & 63;
    bool head; int run_end;
    run_bounds(r, lane, &head, &run_end);
    if (live && head) atomicAdd(size + r, run_end - lane + 1);
}

// 1 at every root whose cluster is kept, 0 elsewhere, over the whole capacity (the scan's length is the capacity)
__global__ void __launch_bounds__(256) flag_kernel(const int *__restrict__ root, const int *__restrict__ size, const int64_t *__restrict__ totals, int64_t mv,
                                                  int min_voxels, int64_t *__restrict__ flag) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= mv) return;
    const int64_t total = totals[0];
    flag[i] = (total <= mv && i < total && root[i] == (int)i && size[i] >= min_voxels) ? 1 : 0;
}

// per voxel: its cluster's row; per kept cluster: count and coordinate sums (integer atomics: exact, whatever the order)
__global__ void __launch_bounds__(256) rows_kernel(const int64_t *__restrict__ vox, const int *__restrict__ root, const int64_t *__restrict__ flag,
                                                  const int64_t *__restrict__ row, const int64_t *__restrict__ totals, int64_t mv, int64_t mc, BitGrid g,
                                                  int64_t *__restrict__ sums, double *__restrict__ clusters, int64_t *__restrict__ cluster_counts,
                                                  int *__restrict__ voxel_cluster) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t total = totals[0];
    if (total > mv) return;                                          // (uniform)
    const bool live = i < total;
    int64_t r = -1, x = 0, y = 0, z = 0;
    if (live) {
        const int rt = root[i];
        r = flag[rt] ? row[rt] : -1;
        if (voxel_cluster) voxel_cluster[i] = (int)r;
        const int64_t id = vox[i];
        const int64_t c = id / g.n_vox, lin = id - c * g.n_vox;
        z = lin % g.Z; y = (lin / g.Z) % g.Y; x = lin / ((int64_t)g.Z * g.Y);
        if (r >= 0 && rt == (int)i) {                                // the cluster's root: its first voxel
            atomicAdd(reinterpret_cast<unsigned long long *>(cluster_counts + c), 1ull);
            if (r < mc) clusters[r * 5] = (double)c;
        }
    }
    const int lane = threadIdx.x & 63;
    bool head; int run_end;
    run_bounds(r, lane, &head, &run_end);
    const int64_t sx = run_sum(x, lane, run_end), sy = run_sum(y, lane, run_end), sz = run_sum(z, lane, run_end);
    if (live && head && r >= 0 && r < mc) {
        unsigned long long *s = reinterpret_cast<unsigned long long *>(sums + r * 4);
        atomicAdd(s, (unsigned long long)(run_end - lane + 1));
        atomicAdd(s + 1, (unsigned long long)sx);
        atomicAdd(s + 2, (unsigned long long)sy);
        atomicAdd(s + 3, (unsigned long long)sz);
    }
}

__global__ void __launch_bounds__(256) finish_kernel(const int64_t *__restrict__ totals, int64_t mv, int64_t mc, const int64_t *__restrict__ sums,
                                                    double gx, double gy, double gz, double voxel_size, double *__restrict__ clusters,
                                                    int64_t *__restrict__ info) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (totals[0] > mv) return;
    const int64_t found = totals[1];
    if (i == 0) { info[1] = found; info[3] = found > mc ? 1 : 0; }
    if (i >= found || i >= mc) return;
    const double n = (double)sums[i * 4];
    double *out = clusters + i * 5;                                  // [0], the class, is the root's (rows_kernel)
    out[1] = n;
    out[2] = gx + ((double)sums[i * 4 + 1] / n + 0.5) * voxel_size;
    out[3] = gy + ((double)sums[i * 4 + 2] / n + 0.5) * voxel_size;
    out[4] = gz + ((double)sums[i * 4 + 3] / n + 0.5) * voxel_size;
}

// ---------------------------------------------------------------------------------------------------------------- match
// One wave per class.  Lane l owns the ground-truth objects g = l, l + 64, ...: it alone reads and writes gt_match[g], so the "taken" mark needs
// no exchange through memory between lanes.
__global__ void __launch_bounds__(64) match_kernel(const double *__restrict__ clusters, const int64_t *__restrict__ info, int64_t mc, int C,
                                                  const double *__restrict__ gt_locs, const int *__restrict__ gt_class, int G, double thresh,
                                                  int *__restrict__ detected, int *__restrict__ match, int *__restrict__ gt_match) {
    const int c = blockIdx.x, lane = threadIdx.x;
    for (int g = lane; g < G; g += 64) {
        const int k = gt_class[g];
        if (k == c || (c == 0 && (k < 0 || k >= C))) gt_match[g] = -1;
    }
    if (info[2]) {                                                   // no cluster rows were written
        if (lane == 0) detected[c] = 0;
        return;
    }
    const int64_t rows = info[1] < mc ? info[1] : mc;
    // the rows are ordered by class: this class's are [lo, lo + cnt)
    int64_t lo = 0, cnt = 0;
    for (int64_t r = lane; r < rows; r += 64) {
        const int k = (int)clusters[r * 5];
        lo += k < c ? 1 : 0;
        cnt += k == c ? 1 : 0;
    }
    wave_sum_all_each(lo, cnt);
    int found = 0;
    for (int64_t r = lo; r < lo + cnt; ++r) {
        const double cx = clusters[r * 5 + 2], cy = clusters[r * 5 + 3], cz = clusters[r * 5 + 4];
        double best = 10.0;                                          // eval_pipeline_offline.py:50
        int arg = -1;
        for (int g = lane; g < G; g += 64) {
            if (gt_class[g] != c || gt_match[g] >= 0) continue;
            const double dx = gt_locs[3 * g] - cx, dy = gt_locs[3 * g + 1] - cy, dz = gt_locs[3 * g + 2] - cz;
            const double dist = sqrt((dx * dx + dy * dy) + dz * dz);
            if (dist < thresh && dist < best) { best = dist; arg = g; }      // ascending g, strict: the lowest index of a tie stays
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const double ob = __shfl_xor(best, off, 64);
            const int oa = __shfl_xor(arg, off, 64);
            if (oa >= 0 && (arg < 0 || ob < best || (ob == best && oa < arg))) { best = ob; arg = oa; }
        }
        if (arg >= 0 && (arg & 63) == lane) gt_match[arg] = (int)r;
        if (lane == 0) match[r] = arg;
        found += arg >= 0 ? 1 : 0;
    }
    if (lane == 0) detected[c] = found;
}

}  // namespace
}  // namespace mnf

using namespace mnf;

extern "C" int64_t mnf_object_map_bytes(int32_t n_classes, int32_t res_x, int32_t res_y, int32_t res_z) {
    BitGrid g;
    if (!make_bit_grid(n_classes, res_x, res_y, res_z, &g)) return 0;
    return g.wpp * n_classes * (int64_t)sizeof(uint32_t);
}

extern "C" int mnf_object_map_insert(uint32_t *bits, int32_t n_classes, int32_t res_x, int32_t res_y, int32_t res_z, const float *grid_min_host,
                                     float voxel_size, int32_t first_class, const float *origins, const float *viewdirs, const float *depth,
                                     const float *acc, const float *sem, const void *labels, int32_t label_is_u8, int64_t n_rays,
                                     float min_depth, float max_depth, float min_acc, mnf_stream_t stream) {
    BitGrid g;
    MNF_REQUIRE(n_classes > 0, "object_map_insert: n_classes must be positive (got %d)", n_classes);
    MNF_REQUIRE(res_x > 0 && res_y > 0 && res_z > 0, "object_map_insert: resolution must be positive (got %d x %d x %d)", res_x, res_y, res_z);
    MNF_REQUIRE(make_bit_grid(n_classes, res_x, res_y, res_z, &g), "object_map_insert: resolution %d x %d x %d with %d classes is more than the map indexes",
                res_x, res_y, res_z, n_classes);
    MNF_REQUIRE(voxel_size > 0.0f && voxel_size - voxel_size == 0.0f, "object_map_insert: voxel_size must be positive and finite (got %g)", (double)voxel_size);
    MNF_REQUIRE(first_class >= 0 && first_class < n_classes, "object_map_insert: first_class (%d) outside [0, %d)", first_class, n_classes);
    MNF_REQUIRE(n_rays >= 0, "object_map_insert: n_rays is negative (%lld)", (long long)n_rays);
    MNF_REQUIRE(!(sem && labels), "object_map_insert: both label sources given (sem and labels): exactly one");
    MNF_REQUIRE(sem || labels || n_rays == 0, "object_map_insert: neither label source given (sem or labels): exactly one");
    MNF_REQUIRE(grid_min_host, "object_map_insert: grid_min is null");
    MNF_REQUIRE(min_depth == min_depth && max_depth == max_depth && min_acc == min_acc, "object_map_insert: min_depth, max_depth or min_acc is NaN");
    if (n_rays == 0) return MNF_OK;
    MNF_REQUIRE(bits, "object_map_insert: bits is null");
    MNF_REQUIRE(aligned8(bits), "object_map_insert: bits must be 8-byte aligned");
    MNF_REQUIRE(origins, "object_map_insert: origins is null");
    MNF_REQUIRE(viewdirs, "object_map_insert: viewdirs is null");
    MNF_REQUIRE(depth, "object_map_insert: depth is null");
    int tp = kViewThreads;
    size_t lds = 0;
    if (sem) {
        tp = stage_tile_pixels(n_classes);
        if (tp < 1) {
            set_error("object_map_insert: n_classes = %d is more than one LDS tile holds (%d)", n_classes, kStageBytes / 4 - 1);
            return MNF_ERR_UNSUPPORTED;
        }
        lds = (size_t)tp * (n_classes | 1) * sizeof(float);
    }
    const int64_t tiles = ceil_div(n_rays, tp);
    const int nb = (int)(tiles < kInsertMaxBlocks ? tiles : kInsertMaxBlocks);
    const float inv = 1.0f / voxel_size;
    hipStream_t s = as_stream(stream);
    ProfScope prof("object_map_insert", s);
    hipLaunchKernelGGL(object_map_insert_kernel, dim3(nb), dim3(kViewThreads), lds, s, origins, viewdirs, depth, acc, sem, labels, label_is_u8, n_rays,
                       n_classes, tp, tiles, grid_min_host[0], grid_min_host[1], grid_min_host[2], inv, g, first_class, min_depth, max_depth, min_acc, bits);
    return launch_status("object_map_insert_kernel");
}

extern "C" int mnf_object_map_count(const uint32_t *bits, int32_t n_classes, int32_t res_x, int32_t res_y, int32_t res_z, int64_t *counts,
                                    mnf_stream_t stream) {
    BitGrid g;
    MNF_REQUIRE(make_bit_grid(n_classes, res_x, res_y, res_z, &g), "object_map_count: bad geometry (%d classes, resolution %d x %d x %d)", n_classes, res_x, res_y,
                res_z);
    MNF_REQUIRE(bits, "object_map_count: bits is null");
    MNF_REQUIRE(counts, "object_map_count: counts is null");
    MNF_REQUIRE(n_classes <= 65535, "object_map_count: at most 65535 classes (got %d)", n_classes);
    hipStream_t s = as_stream(stream);
    ProfScope prof("object_map_count", s);
    hipLaunchKernelGGL(object_map_count_kernel, dim3(n_classes), dim3(256), 0, s, bits, g, counts);
    return launch_status("object_map_count_kernel");
}

extern "C" int64_t mnf_object_map_clusters_workspace_bytes(int32_t n_classes, int32_t res_x, int32_t res_y, int32_t res_z, int64_t max_voxels) {
    BitGrid g;
    if (!make_bit_grid(n_classes, res_x, res_y, res_z, &g) || max_voxels < 0 || max_voxels > 0x7fffffff) return 0;
    return carve(nullptr, g, n_classes, max_voxels).bytes;
}

extern "C" int mnf_object_map_clusters(const uint32_t *bits, int32_t n_classes, int32_t res_x, int32_t res_y, int32_t res_z, const float *grid_min_host,
                                       float voxel_size, int32_t link_r2, int32_t min_cluster_voxels, int64_t max_voxels, int64_t max_clusters,
                                       double *clusters, int64_t *cluster_counts, int64_t *info, int64_t *voxel_ids, int32_t *voxel_cluster,
                                       void *workspace, int64_t workspace_bytes, mnf_stream_t stream) {
    BitGrid g;
    MNF_REQUIRE(n_classes > 0, "object_map_clusters: n_classes must be positive (got %d)", n_classes);
    MNF_REQUIRE(res_x > 0 && res_y > 0 && res_z > 0, "object_map_clusters: resolution must be positive (got %d x %d x %d)", res_x, res_y, res_z);
    MNF_REQUIRE(make_bit_grid(n_classes, res_x, res_y, res_z, &g), "object_map_clusters: resolution %d x %d x %d with %d classes is more than the map indexes",
                res_x, res_y, res_z, n_classes);
    MNF_REQUIRE(voxel_size > 0.0f && voxel_size - voxel_size == 0.0f, "object_map_clusters: voxel_size must be positive and finite (got %g)", (double)voxel_size);
    MNF_REQUIRE(link_r2 >= 1 && link_r2 <= 8, "object_map_clusters: link_r2 must lie in 1 .. 8 (got %d)", link_r2);
    MNF_REQUIRE(min_cluster_voxels >= 1, "object_map_clusters: min_cluster_voxels must be at least 1 (got %d)", min_cluster_voxels);
    MNF_REQUIRE(max_voxels >= 0 && max_voxels <= 0x7fffffff, "object_map_clusters: max_voxels outside [0, 2^31) (got %lld)", (long long)max_voxels);
    MNF_REQUIRE(max_clusters >= 0 && max_clusters <= 0x7fffffff, "object_map_clusters: max_clusters outside [0, 2^31) (got %lld)", (long long)max_clusters);
    MNF_REQUIRE(bits, "object_map_clusters: bits is null");
    MNF_REQUIRE(grid_min_host, "object_map_clusters: grid_min is null");
    MNF_REQUIRE(clusters || max_clusters == 0, "object_map_clusters: clusters is null");
    MNF_REQUIRE(cluster_counts, "object_map_clusters: cluster_counts is null");
    MNF_REQUIRE(info, "object_map_clusters: info is null");
    MNF_REQUIRE(workspace, "object_map_clusters: workspace is null");
    MNF_REQUIRE(aligned8(workspace), "object_map_clusters: workspace must be 8-byte aligned");
    const ClusterWs w = carve(workspace, g, n_classes, max_voxels);
    MNF_REQUIRE(workspace_bytes >= w.bytes, "object_map_clusters: workspace too small (%lld < %lld bytes)", (long long)workspace_bytes, (long long)w.bytes);
    Offsets offs;
    offs.n = 0;
    for (int dx = 0; dx <= 2; ++dx)
        for (int dy = -2; dy <= 2; ++dy)
            for (int dz = -2; dz <= 2; ++dz) {
                const bool forward = dx > 0 || (dx == 0 && (dy > 0 || (dy == 0 && dz > 0)));       // the half with a positive linear offset
                if (!forward || dx * dx + dy * dy + dz * dz > link_r2) continue;
                offs.d[offs.n][0] = (signed char)dx; offs.d[offs.n][1] = (signed char)dy; offs.d[offs.n][2] = (signed char)dz;
                ++offs.n;
            }
    hipStream_t s = as_stream(stream);
    ProfScope prof("object_map_clusters", s);
    const int64_t nw = g.wpp * n_classes, mv = max_voxels, mc = max_clusters;
    hipLaunchKernelGGL(popcount_words_kernel, dim3(blocks_for(nw)), dim3(256), 0, s, bits, g, nw, w.wordcnt);
    int rc = launch_status("popcount_words_kernel");
    if (rc) return rc;
    rc = mnf_exclusive_scan_i64(w.wordcnt, nw, w.prefix, w.totals, w.scan, scan_bytes(nw), stream);
    if (rc) return rc;
    const int64_t init_n = mc * 4 > n_classes ? mc * 4 : n_classes;
    hipLaunchKernelGGL(clusters_init_kernel, dim3(blocks_for(init_n)), dim3(256), 0, s, w.totals, mv, mc, n_classes, w.sums, cluster_counts, info);
    rc = launch_status("clusters_init_kernel");
    if (rc || mv == 0) return rc;                                    // no capacity: info says whether anything was set
    hipLaunchKernelGGL(enumerate_kernel, dim3(blocks_for(nw)), dim3(256), 0, s, bits, g, nw, w.prefix, w.totals, mv, w.vox, w.parent, w.size, voxel_ids);
    hipLaunchKernelGGL(link_kernel, dim3(blocks_for(mv)), dim3(256), 0, s, bits, g, w.prefix, w.totals, mv, w.vox, offs, w.parent);
    hipLaunchKernelGGL(roots_kernel, dim3(blocks_for(mv)), dim3(256), 0, s, w.parent, w.totals, mv, w.root, w.size);
    hipLaunchKernelGGL(flag_kernel, dim3(blocks_for(mv)), dim3(256), 0, s, w.root, w.size, w.totals, mv, min_cluster_voxels, w.flag);
    rc = launch_status("flag_kernel");
    if (rc) return rc;
    rc = mnf_exclusive_scan_i64(w.flag, mv, w.row, w.totals + 1, w.scan, scan_bytes(mv), stream);
    if (rc) return rc;
    hipLaunchKernelGGL(rows_kernel, dim3(blocks_for(mv)), dim3(256), 0, s, w.vox, w.root, w.flag, w.row, w.totals, mv, mc, g, w.sums, clusters, cluster_counts,
                       voxel_cluster);
    hipLaunchKernelGGL(finish_kernel, dim3(blocks_for(mc)), dim3(256), 0, s, w.totals, mv, mc, w.sums, (double)grid_min_host[0], (double)grid_min_host[1],
                       (double)grid_min_host[2], (double)voxel_size, clusters, info);
    return launch_status("finish_kernel");
}

extern "C" int mnf_object_map_match(const double *clusters, const int64_t *info, int64_t max_clusters, int32_t n_classes, const double *gt_locs,
                                    const int32_t *gt_class, int32_t n_gt, double det_dist_thresh, int32_t *detected, int32_t *match, int32_t *gt_match,
                                    mnf_stream_t stream) {
    MNF_REQUIRE(n_classes > 0 && n_classes <= 65535, "object_map_match: n_classes outside 1 .. 65535 (got %d)", n_classes);
    MNF_REQUIRE(max_clusters >= 0 && max_clusters <= 0x7fffffff, "object_map_match: max_clusters outside [0, 2^31) (got %lld)", (long long)max_clusters);
    MNF_REQUIRE(n_gt >= 0, "object_map_match: n_gt is negative (%d)", n_gt);
    MNF_REQUIRE(det_dist_thresh == det_dist_thresh, "object_map_match: det_dist_thresh is NaN");
    MNF_REQUIRE(clusters || max_clusters == 0, "object_map_match: clusters is null");
    MNF_REQUIRE(info, "object_map_match: info is null");
    MNF_REQUIRE(gt_locs || n_gt == 0, "object_map_match: gt_locs is null");
    MNF_REQUIRE(gt_class || n_gt == 0, "object_map_match: gt_class is null");
    MNF_REQUIRE(gt_match || n_gt == 0, "object_map_match: gt_match is null");
    MNF_REQUIRE(detected, "object_map_match: detected is null");
    MNF_REQUIRE(match || max_clusters == 0, "object_map_match: match is null");
    hipStream_t s = as_stream(stream);
    ProfScope prof("object_map_match", s);
    hipLaunchKernelGGL(match_kernel, dim3(n_classes), dim3(64), 0, s, clusters, info, max_clusters, n_classes, gt_locs, gt_class, n_gt, det_dist_thresh, detected,
                       match, gt_match);
    return launch_status("match_kernel");
}
