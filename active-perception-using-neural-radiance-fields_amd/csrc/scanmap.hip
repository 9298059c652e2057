// The planner's cost map and visit counts from depth scan lines, and the goal draw of sample_traj, on the device (gfx950).
//   mnf_scan_map_update    <- planning/planning_funcs.py:192-219 (update_cost_map) over perception/data_proc/depth_to_grid.py:31-73 (bresenham),
//                             :142-182 (generate_ray_casting_grid_map); the callers are scripts/pipeline.py:272-292, :1115-1138, :1171-1189
//   mnf_planner_goal_map   <- planning/planning_funcs.py:262-276 (vm), :296-298 (free_indices)
//   mnf_planner_goal_pick  <- planning/planning_funcs.py:296-326 (the draw-and-reject loop)
// The definition is in include/mi355nerf.h ("planner cost map").  The one deliberate difference from the reference: a cell with a negative
// index is skipped and its beam counted, where the reference wraps round through Python's negative indexing or raises.
//
// scan_update_kernel: one workgroup of 1024 threads per view, the view's key plane [nx][nz] uint32 in dynamic LDS (at the planner's cap
// (nx + 2)(nz + 2) <= 40 000 that is below 160 000 B of the CU's 163 840).  The reference draws beam after beam and lets the later write win; here
// every write of beam j carries the key 2 j + occ + 1 (occ = 0 for a free cell, 1 for a stamped one) and writes are combined with ds_max_u32, so a
// cell ends with the key of the write the serial loop would have made last, whatever the schedule: key - 1 = 2 j + occ orders the beams, and within
// a beam the stamp after the walk.  A wave takes 64 beams: lane l works out the end cell of beam l (float64, every operation rounded on its
// own), then the wave draws the 64 beams one after the other with one lane per Bresenham column.  Column k of the reference's walk has the closed
// form y = y1 + ystep ((k |dy| - e0 + dx - 1) / dx), e0 = dx / 2 (the error term stays in [0, dx), so the number of steps taken before column k is a
// ceiling division), so no lane depends on another, and a beam is entered at the border of the grid: its work is bounded by the grid, not by
// the depth.  When all beams are drawn the workgroup folds its plane into the map: a global max of 2 (v + 1) + occ per cell orders the views, and a
// cell the view left free adds one to its visit count.  scan_resolve_kernel then writes the cost code of every cell a view of this call touched.
// No floating-point value is ever accumulated; every atomic is an integer max or add, so the result does not depend on the schedule.
//
// goal_map_kernel: one workgroup.  The minimum visit count over free cells (integer), vm from the caller's decay table, and the goal list by an
// ordered compaction over tiles of 1024 cells (map_dev.h: block_rank): row-major order, the same bytes every time.
#include "map_dev.h"

#include <cmath>

namespace mnf {
namespace {

constexpr int kScanThreads = 1024;                    // the cap (nx + 2)(nz + 2) <= kMaxBorderedCells and kUnreached are the planner's: map_dev.h
constexpr int32_t kFar = 1 << 30;                     // an end cell or centre beyond +-kFar is not drawn
constexpr int32_t kMaxBeams = 1 << 24;                // keys 2 j + 2 stay far below 2^32
constexpr int32_t kMaxViews = 1 << 20;                // view keys 2 (v + 1) + 1 likewise
constexpr double kTwoPi = 2.0 * 3.141592653589793;    // 2 * np.pi

// numpy's float remainder for a positive divisor: fmod, then the divisor's sign
__device__ __forceinline__ double py_mod_pos(double a, double b) {
    double m = fmod(a, b);
    if (m != 0.0) { if (m < 0.0) m += b; } else m = 0.0;
    return m;
}

__global__ void __launch_bounds__(kScanThreads) scan_update_kernel(const float *__restrict__ depth, int H, int W, const double *__restrict__ align,
                                                                   const double *__restrict__ yaw, const double *__restrict__ loc,
                                                                   const int32_t *__restrict__ centre, double min_x, double min_y, double res, int nx, int nz,
                                                                   uint32_t *__restrict__ last, int32_t *__restrict__ visits,
                                                                   unsigned long long *__restrict__ info) {
    extern __shared__ uint32_t plane[];               // [nx][nz] keys of this view
    __shared__ unsigned int tally[4];                 // beams: with a negative cell, non-finite depth, far, drawn
    const int tid = threadIdx.x, v = blockIdx.x, lane = tid & 63, wave = tid >> 6;
    const int cells = nx * nz;
    for (int i = tid; i < cells; i += kScanThreads) plane[i] = 0;
    if (tid < 4) tally[tid] = 0;
    __syncthreads();
    const float *row = depth + ((int64_t)v * H + H / 2) * W;
    const double yaw_v = yaw[v], loc_x = loc[2 * v], loc_z = loc[2 * v + 1];
    const int cx = centre[2 * v], cy = centre[2 * v + 1];
    const bool centre_far = cx > kFar || cx < -kFar || cy > kFar || cy < -kFar;
    for (int j0 = wave * 64; j0 < W; j0 += kScanThreads) {
        // lane l: the end cell of beam j0 + l.  status 0 = draw, 1 = negative cell (drawn), 2 = non-finite depth, 3 = far, 4 = no beam
        const int jm = j0 + lane;
        int my_ix = 0, my_iy = 0, my_status = 4;
        if (jm < W) {
            const double d = (double)row[jm];
            if (!isfinite(d)) my_status = 2;
            else {
                const double a = py_mod_pos(align[jm] + yaw_v, kTwoPi);
                const double ox = sin(-a) * d + loc_x;
                const double oy = (-cos(-a)) * d + loc_z;
                const double fx = rint((ox - min_x) / res), fy = rint((oy - min_y) / res);       // round-half-even, as Python's round
                if (centre_far || !(fabs(fx) <= (double)kFar && fabs(fy) <= (double)kFar)) my_status = 3;
                else {
                    my_ix = (int)fx; my_iy = (int)fy;
                    my_status = (my_ix < 0 || my_iy < 0 || cx < 0 || cy < 0) ? 1 : 0;
                }
            }
            if (my_status < 2) atomicAdd(&tally[3], 1u);
            if (my_status >= 1 && my_status <= 3) atomicAdd(&tally[my_status - 1], 1u);
        }
        const int n_here = W - j0 < 64 ? W - j0 : 64;
        for (int b = 0; b < n_here; ++b) {
            const int status = __shfl(my_status, b, 64), ix = __shfl(my_ix, b, 64), iy = __shfl(my_iy, b, 64);
            if (status >= 2) continue;                                                            // (wave-uniform)
            const uint32_t key_free = 2u * (uint32_t)(j0 + b) + 1u, key_occ = key_free + 1u;
            // depth_to_grid.py:31-73: steep swap, end swap, the walk from the low end
            int64_t x1 = cx, y1 = cy, x2 = ix, y2 = iy;
            const int64_t adx0 = x2 > x1 ? x2 - x1 : x1 - x2, ady0 = y2 > y1 ? y2 - y1 : y1 - y2;
            const bool steep = ady0 > adx0;
            if (steep) { int64_t t = x1; x1 = y1; y1 = t; t = x2; x2 = y2; y2 = t; }
            if (x1 > x2) { int64_t t = x1; x1 = x2; x2 = t; t = y1; y1 = y2; y2 = t; }
            const int64_t dx = x2 - x1, ady = y2 > y1 ? y2 - y1 : y1 - y2, e0 = dx >> 1, ystep = y1 < y2 ? 1 : -1;
            const int64_t n_major = steep ? nz : nx, n_minor = steep ? nx : nz;
            const int64_t k_lo = x1 < 0 ? -x1 : 0, k_hi = dx < n_major - 1 - x1 ? dx : n_major - 1 - x1;        // columns inside the grid
            const bool narrow = dx < 32768;                                                       // k |dy| + dx < 2^31: 32-bit division
            for (int64_t k = k_lo + lane; k <= k_hi; k += 64) {
                int64_t s = 0;
                if (dx > 0) s = narrow ? (int64_t)((uint32_t)(k * ady - e0 + dx - 1) / (uint32_t)dx) : (k * ady - e0 + dx - 1) / dx;
                const int64_t y = y1 + ystep * s, x = x1 + k;
                if (y < 0 || y >= n_minor) continue;
                const int cell = steep ? (int)(y * nz + x) : (int)(x * nz + y);
                atomicMax(&plane[cell], key_free);
            }
            if (lane < 4) {                                                                       // depth_to_grid.py:175-182: the 2 x 2 stamp
                const int px = ix + (lane & 1), py = iy + (lane >> 1);
                if (px >= 0 && px < nx && py >= 0 && py < nz) atomicMax(&plane[px * nz + py], key_occ);
            }
        }
    }
    __syncthreads();
    const uint32_t view_key = 2u * ((uint32_t)v + 1u);
    for (int i = tid; i < cells; i += kScanThreads) {
        const uint32_t key = plane[i];
        if (key == 0) continue;
        const uint32_t occ = (key - 1u) & 1u;
        atomicMax(&last[i], view_key + occ);
        if (!occ) atomicAdd(&visits[i], 1);
    }
    if (tid < 4 && tally[tid]) atomicAdd(&info[tid], (unsigned long long)tally[tid]);
}

__global__ void __launch_bounds__(256) scan_resolve_kernel(const uint32_t *__restrict__ last, int32_t *__restrict__ cost, int cells) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= cells) return;
    const uint32_t l = last[i];
    if (l) cost[i] = (l & 1u) ? 2 : 1;
}

__global__ void __launch_bounds__(kScanThreads) goal_map_kernel(const int32_t *__restrict__ blocked, const int32_t *__restrict__ visits,
                                                                const uint32_t *__restrict__ field, int nx, int nz, const double *__restrict__ decay,
                                                                int n_decay, double *__restrict__ vm, int32_t *__restrict__ cells_out,
                                                                int64_t *__restrict__ count) {
    __shared__ int least;
    const int tid = threadIdx.x, lane = tid & 63, cells = nx * nz;
    if (tid == 0) least = 0x7fffffff;
    __syncthreads();
    int mine = 0x7fffffff;
    for (int i = tid; i < cells; i += kScanThreads)
        if (blocked[i] <= 0) { const int c = visits[i]; mine = c < mine ? c : mine; }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { const int o = __shfl_down(mine, off, 64); mine = o < mine ? o : mine; }
    if (lane == 0 && mine != 0x7fffffff) atomicMin(&least, mine);
    __syncthreads();
    const int lo = least;
    int n = 0;                                                                                    // the cells listed so far (uniform)
    for (int t0 = 0; t0 < cells; t0 += kScanThreads) {
        const int i = t0 + tid;
        bool keep = false;
        if (i < cells) {
            double val = -1.0;                                                                    // planning_funcs.py:269
            if (blocked[i] <= 0) {                                                                // :270-276
                const int64_t m = (int64_t)visits[i] - (int64_t)lo;
                val = (m >= 0 && m < (int64_t)n_decay) ? decay[m] : 0.0;                          // m >= 0 by the choice of `lo`
            }
            vm[i] = val;
            keep = val >= 0.0 && (field == nullptr || field[i] != kUnreached);                    // :298, and the goals planning() answers
        }
        int total;
        const int pos = n + block_rank<kScanThreads>(keep, &total);
        if (keep) {
            const int x = i / nz;
            cells_out[2 * pos] = x; cells_out[2 * pos + 1] = i - x * nz;
        }
        n += total;
    }
    for (int i = n + tid; i < cells; i += kScanThreads) { cells_out[2 * i] = -1; cells_out[2 * i + 1] = -1; }
    if (tid == 0) count[0] = n;
}

__global__ void __launch_bounds__(256) goal_pick_kernel(const int32_t *__restrict__ cells, const int64_t *__restrict__ count, int64_t max_cells,
                                                        const double *__restrict__ u, int64_t n_draws, int32_t *__restrict__ goals) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_draws) return;
    int64_t n = count[0];
    n = n > max_cells ? max_cells : n;
    int gx = -1, gy = -1;
    if (n > 0) {
        const double t = floor(u[i] * (double)n);
        int64_t k = t >= 0.0 ? (t < (double)n ? (int64_t)t : n - 1) : 0;                          // NaN and negatives: the first cell
        gx = cells[2 * k]; gy = cells[2 * k + 1];
    }
    goals[2 * i] = gx; goals[2 * i + 1] = gy;
}

}  // namespace
}  // namespace mnf

using namespace mnf;

extern "C" int64_t mnf_scan_map_bytes(int32_t nx, int32_t nz) {
    if (!planner_geometry_ok(nx, nz)) return 0;
    return 3 * (int64_t)nx * nz * (int64_t)sizeof(int32_t);
}

extern "C" int mnf_scan_map_update(void *state, int32_t nx, int32_t nz, const float *depth, int32_t n_views, int32_t height, int32_t width,
                                   const double *align, const double *yaw, const double *loc, const int32_t *centre, const double *aabb_host,
                                   double res, int64_t *info, mnf_stream_t stream) {
    MNF_REQUIRE(nx > 0 && nz > 0, "scan_map_update: the grid size must be positive (got %d x %d)", nx, nz);
    MNF_REQUIRE(planner_geometry_ok(nx, nz), "scan_map_update: a %d x %d grid is more than the %lld bordered cells one workgroup's LDS holds", nx, nz,
                (long long)kMaxBorderedCells);
    MNF_REQUIRE(n_views >= 0 && n_views <= kMaxViews, "scan_map_update: n_views outside [0, %d] (got %d)", kMaxViews, n_views);
    MNF_REQUIRE(height > 0, "scan_map_update: height must be positive (got %d)", height);
    MNF_REQUIRE(width > 0 && width <= kMaxBeams, "scan_map_update: width outside [1, %d] (got %d)", kMaxBeams, width);
    MNF_REQUIRE(aabb_host, "scan_map_update: aabb_host is null");
    for (int k = 0; k < 6; ++k) MNF_REQUIRE(std::isfinite(aabb_host[k]), "scan_map_update: aabb[%d] is not finite", k);
    MNF_REQUIRE(std::isfinite(res) && res > 0.0, "scan_map_update: res must be finite and positive (got %g)", res);
    MNF_REQUIRE(state, "scan_map_update: state is null");
    MNF_REQUIRE(info, "scan_map_update: info is null");
    MNF_REQUIRE(depth || n_views == 0, "scan_map_update: depth is null");
    MNF_REQUIRE(align || n_views == 0, "scan_map_update: align is null");
    MNF_REQUIRE(yaw || n_views == 0, "scan_map_update: yaw is null");
    MNF_REQUIRE(loc || n_views == 0, "scan_map_update: loc is null");
    MNF_REQUIRE(centre || n_views == 0, "scan_map_update: centre is null");
    MNF_REQUIRE(aligned8(info) && aligned8(align) && aligned8(yaw) && aligned8(loc), "scan_map_update: info, align, yaw and loc must be 8-byte aligned");
    MNF_REQUIRE(aligned4(state) && aligned4(centre) && aligned4(depth), "scan_map_update: state, centre and depth must be 4-byte aligned");
    if (n_views == 0) return MNF_OK;
    const int cells = nx * nz;
    int32_t *cost = static_cast<int32_t *>(state), *visits = cost + cells;
    uint32_t *last = reinterpret_cast<uint32_t *>(cost + 2 * (int64_t)cells);
    hipStream_t s = as_stream(stream);
    MNF_HIP(hipFuncSetAttribute((const void *)scan_update_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kMaxBorderedCells * 4));
    ProfScope prof("scan_map_update", s);
    MNF_HIP(hipMemsetAsync(last, 0, (size_t)cells * sizeof(uint32_t), s));
    hipLaunchKernelGGL(scan_update_kernel, dim3((unsigned)n_views), dim3(kScanThreads), (size_t)cells * sizeof(uint32_t), s, depth, height, width, align, yaw,
                       loc, centre, aabb_host[2], aabb_host[0], res, nx, nz, last, visits, reinterpret_cast<unsigned long long *>(info));
    if (int rc = launch_status("scan_update_kernel")) return rc;
    hipLaunchKernelGGL(scan_resolve_kernel, dim3((unsigned)ceil_div(cells, 256)), dim3(256), 0, s, last, cost, cells);
    return launch_status("scan_resolve_kernel");
}

extern "C" int mnf_planner_goal_map(const int32_t *blocked, const int32_t *visits, const uint32_t *field, int32_t nx, int32_t nz, const double *decay,
                                    int32_t n_decay, double *vm, int32_t *cells, int64_t *count, mnf_stream_t stream) {
    MNF_REQUIRE(nx > 0 && nz > 0, "planner_goal_map: the map size must be positive (got %d x %d)", nx, nz);
    MNF_REQUIRE(planner_geometry_ok(nx, nz), "planner_goal_map: a %d x %d map is beyond the planner's cap of %lld bordered cells", nx, nz,
                (long long)kMaxBorderedCells);
    MNF_REQUIRE(n_decay >= 1, "planner_goal_map: n_decay must be at least 1 (got %d)", n_decay);
    MNF_REQUIRE(blocked, "planner_goal_map: blocked is null");
    MNF_REQUIRE(visits, "planner_goal_map: visits is null");
    MNF_REQUIRE(decay, "planner_goal_map: decay is null");
    MNF_REQUIRE(vm, "planner_goal_map: vm is null");
    MNF_REQUIRE(cells, "planner_goal_map: cells is null");
    MNF_REQUIRE(count, "planner_goal_map: count is null");
    MNF_REQUIRE(aligned8(decay) && aligned8(vm) && aligned8(count), "planner_goal_map: decay, vm and count must be 8-byte aligned");
    hipStream_t s = as_stream(stream);
    ProfScope prof("planner_goal_map", s);
    hipLaunchKernelGGL(goal_map_kernel, dim3(1), dim3(kScanThreads), 0, s, blocked, visits, field, nx, nz, decay, n_decay, vm, cells, count);
    return launch_status("goal_map_kernel");
}

extern "C" int mnf_planner_goal_pick(const int32_t *cells, const int64_t *count, int64_t max_cells, const double *u, int64_t n_draws, int32_t *goals,
                                     mnf_stream_t stream) {
    MNF_REQUIRE(max_cells >= 0 && max_cells <= kMaxBorderedCells, "planner_goal_pick: max_cells outside [0, %lld] (got %lld)", (long long)kMaxBorderedCells,
                (long long)max_cells);
    MNF_REQUIRE(n_draws >= 0 && n_draws <= (int64_t)0x7fffffff, "planner_goal_pick: n_draws outside [0, 2^31) (got %lld)", (long long)n_draws);
    MNF_REQUIRE(count, "planner_goal_pick: count is null");
    MNF_REQUIRE(cells || max_cells == 0, "planner_goal_pick: cells is null");
    MNF_REQUIRE(u || n_draws == 0, "planner_goal_pick: u is null");
    MNF_REQUIRE(goals || n_draws == 0, "planner_goal_pick: goals is null");
    MNF_REQUIRE(aligned8(count) && aligned8(u), "planner_goal_pick: count and u must be 8-byte aligned");
    if (n_draws == 0) return MNF_OK;
    hipStream_t s = as_stream(stream);
    ProfScope prof("planner_goal_pick", s);
    hipLaunchKernelGGL(goal_pick_kernel, dim3((unsigned)ceil_div(n_draws, 256)), dim3(256), 0, s, cells, count, max_cells, u, n_draws, goals);
    return launch_status("goal_pick_kernel");
}
