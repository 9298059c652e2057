// The planner's grid search on the device (gfx950): single-source shortest-path fields over a small 8-connected map, and paths read out of them.
//   mnf_path_field  <- planning/dijkstra.py:72-182 (Dijkstra.planning), :194-215 (verify_node), :247-260 (get_motion_model)
//   mnf_path_trace  <- planning/dijkstra.py:170-182 (calc_final_path); one field answers every goal of planning_funcs.py:288-326 (sample_traj)
//
// A label is the uint32 (a << 16) | b of the cheapest way to a cell: a straight and b diagonal moves, cost a + b sqrt(2).  Labels are ordered by
// the exact sign of da + db sqrt(2) in integers (include/mi355nerf.h has the definition); no kernel here does floating-point work, and no cost is
// ever built by adding move after move.
//
// path_field_kernel: one workgroup of 1024 threads per (map, source).  The labels sit in dynamic LDS, [nx + 2][ny + 2] words with a one-cell border
// that is never reached, so the relaxation tests no bounds: at the cap, (nx + 2)(ny + 2) = 40 000 words = 160 000 B of the CU's 163 840, which
// leaves no room for a second plane: a cell that may never be entered (blocked, or beyond the limits) carries the label 0xFFFFFFFE instead, reads
// as "not reached" for its neighbours and is written out as 0xFFFFFFFF.  The row pitch is ny + 2 without padding: the lanes of a wave take
// consecutive cells of a row of the swept box, so each of the nine ds_read_b32 of a cell reads consecutive words (bank = word mod 32), conflict-free
// but for the one place where a wave wraps to the next row (2-way there); a pad would not fit at the cap.
// A sweep relaxes cells to the minimum over their 8 neighbours of label + move, in place and unsynchronised: within a sweep a cell is written by the
// one thread that owns it, labels only decrease, each is one aligned 32-bit word, and the fixpoint is unique, so the result does not depend on the
// schedule.  Sweep s + 1 covers the bounding box of the cells sweep s lowered, grown by one: a cell whose 8 neighbours all kept their labels since it
// was last relaxed cannot be lowered, so nothing outside that box can.  (On open floor the box is that of the reached cells, less what has
// settled on its rim; in corridors it is a few cells around the front.)  After sweep k every cell whose cheapest way has at most k moves is final; a
// way has at most nx ny - 1 moves, so sweep nx ny at the latest lowers nothing.  The loop ends at the first sweep that lowers nothing and, as a guard
// for a shared GPU against a logic error that would never end, after nx ny sweeps whatever happens (info = -1 then).
//
// path_trace_kernel: one lane per goal walks the field in global memory (at most 160 KB per field: L2 hits) by the rule of the header.
#include "map_dev.h"

namespace mnf {
namespace {

constexpr int kFieldThreads = 1024;
constexpr uint32_t kNoEntry = 0xFFFFFFFEu;            // LDS only: blocked or beyond the limits (kUnreached and the cap: map_dev.h)
constexpr uint32_t kStraight = 0x10000u, kDiagonal = 1u;
constexpr int kEmptyLo = 0x7fffffff;                 // an empty box: lo = kEmptyLo, hi = -1

// exact: is a_p + b_p sqrt(2) < a_q + b_q sqrt(2)?  Where the signs of da and db agree, that sign; otherwise da^2 against 2 db^2.  The two "not
// reached" labels need no case of their own: both halves of 0xFFFFFFFF and 0xFFFFFFFE exceed those of any label a field holds (a, b <= nx ny - 1 <
// 39 204), so they order as +infinity through the agreeing signs.  Where the signs differ both labels are a field's, |da|, |db| < 39 204, and
// da^2 and 2 db^2 stay below 2^32: one full-rate 24-bit multiply each.  Never equal: sqrt(2) is irrational.
__device__ __forceinline__ bool label_less(uint32_t p, uint32_t q) {
    const int da = (int)(p >> 16) - (int)(q >> 16), db = (int)(p & 0xffffu) - (int)(q & 0xffffu);
    const uint32_t a2 = (uint32_t)__mul24(da, da), b2 = (uint32_t)__mul24(db, db) << 1;
    const bool mixed = da < 0 ? a2 > b2 : a2 < b2;
    return (da <= 0 && db <= 0) ? (da | db) != 0 : (da >= 0 && db >= 0) ? false : mixed;
}

__device__ __forceinline__ uint32_t label_min(uint32_t p, uint32_t q) { return label_less(q, p) ? q : p; }

__global__ void __launch_bounds__(kFieldThreads) path_field_kernel(const int32_t *__restrict__ blocked, int64_t map_stride, int nx, int ny, int lim_x, int lim_y,
                                                                   const int32_t *__restrict__ sources, uint32_t *__restrict__ field,
                                                                   int64_t *__restrict__ info) {
    extern __shared__ uint32_t lab[];                 // [nx + 2][ny + 2]
    __shared__ int box[2][4];                         // x0, x1, y0, y1 (inclusive) of the cells to sweep: [s & 1] is read by sweep s, the other one grown
    __shared__ int reached;
    const int tid = threadIdx.x, b = blockIdx.x;
    const int P = ny + 2, cells = nx * ny;
    const int sx = sources[2 * b], sy = sources[2 * b + 1];
    uint32_t *out = field + (int64_t)b * cells;
    if ((unsigned)sx >= (unsigned)nx || (unsigned)sy >= (unsigned)ny) {               // (uniform) a source outside the map reaches nothing
        for (int i = tid; i < cells; i += kFieldThreads) out[i] = kUnreached;
        if (tid == 0) { info[2 * b] = 0; info[2 * b + 1] = 0; }
        return;
    }
    const int32_t *map = blocked + (int64_t)b * map_stride;
    for (int i = tid; i < (nx + 2) * P; i += kFieldThreads) {
        const int xb = i / P, x = xb - 1, y = i - xb * P - 1;
        uint32_t v = kUnreached;                                                      // the border
        if ((unsigned)x < (unsigned)nx && (unsigned)y < (unsigned)ny) {
            v = (x < lim_x && y < lim_y && map[x * ny + y] == 0) ? kUnreached : kNoEntry;
            if (x == sx && y == sy) v = 0;                                            // the source is never verified
        }
        lab[i] = v;
    }
    if (tid == 0) {
        box[1][0] = sx > 0 ? sx - 1 : 0; box[1][1] = sx < nx - 1 ? sx + 1 : nx - 1;   // sweep 1: the cells around the source
        box[1][2] = sy > 0 ? sy - 1 : 0; box[1][3] = sy < ny - 1 ? sy + 1 : ny - 1;
        box[0][0] = kEmptyLo; box[0][1] = -1; box[0][2] = kEmptyLo; box[0][3] = -1;
        reached = 0;
    }
    __syncthreads();
    int sweeps = 0;
    bool fixpoint = false;
    for (int s = 1; s <= cells; ++s) {
        int *cur = box[s & 1], *next = box[(s & 1) ^ 1];
        const int x0 = cur[0], x1 = cur[1], y0 = cur[2], y1 = cur[3];
        __syncthreads();                              // everyone holds this sweep's box; `next` is empty
        if (tid == 0) { cur[0] = kEmptyLo; cur[1] = -1; cur[2] = kEmptyLo; cur[3] = -1; }        // the box sweep s + 1 grows
        // thread t takes the box's cells t, t + 1024, ... in row-major order: one division per sweep, none per cell
        const int bh = y1 - y0 + 1, bw = x1 - x0 + 1, step_q = kFieldThreads / bh, step_r = kFieldThreads - step_q * bh;
        int q = tid / bh, r = tid - q * bh;
        int cx0 = kEmptyLo, cx1 = -1, cy0 = kEmptyLo, cy1 = -1;                       // the cells this thread lowered
        while (q < bw) {
            const int x = x0 + q, y = y0 + r;
            q += step_q; r += step_r;                                                 // the cell 1024 further on
            if (r >= bh) { r -= bh; ++q; }
            uint32_t *c = lab + (x + 1) * P + (y + 1);
            const uint32_t mine = *c;
            if (mine == kNoEntry || mine == 0) continue;
            const uint32_t ms = label_min(label_min(c[P], c[1]), label_min(c[-P], c[-1]));
            const uint32_t md = label_min(label_min(c[P + 1], c[P - 1]), label_min(c[-P + 1], c[-P - 1]));
            const uint32_t cand = label_min(ms >= kNoEntry ? kUnreached : ms + kStraight, md >= kNoEntry ? kUnreached : md + kDiagonal);
            if (label_less(cand, mine)) {
                *c = cand;
                cx0 = x < cx0 ? x : cx0; cx1 = x > cx1 ? x : cx1;
                cy0 = y < cy0 ? y : cy0; cy1 = y > cy1 ? y : cy1;
            }
        }
        if (cx1 >= 0) {                               // only the 8 neighbours of a lowered cell can be lowered by the next sweep
            const int g0 = cx0 > 0 ? cx0 - 1 : 0, g1 = cx1 < nx - 1 ? cx1 + 1 : nx - 1, h0 = cy0 > 0 ? cy0 - 1 : 0, h1 = cy1 < ny - 1 ? cy1 + 1 : ny - 1;
            if (g0 < next[0]) atomicMin(next + 0, g0);                                // a stale read only repeats the atomic
            if (g1 > next[1]) atomicMax(next + 1, g1);
            if (h0 < next[2]) atomicMin(next + 2, h0);
            if (h1 > next[3]) atomicMax(next + 3, h1);
        }
        __syncthreads();
        sweeps = s;
        if (next[1] < 0) { fixpoint = true; break; }  // (uniform) nothing was lowered; `next` is reset only behind the next barrier
    }
    int mine = 0;
    for (int i = tid; i < cells; i += kFieldThreads) {                                // coalesced, without the border
        const int x = i / ny, y = i - x * ny;
        uint32_t v = lab[(x + 1) * P + (y + 1)];
        if (v >= kNoEntry) v = kUnreached; else ++mine;
        out[i] = v;
    }
    mine = wave_sum(mine);
    if ((tid & 63) == 0 && mine) atomicAdd(&reached, mine);
    __syncthreads();
    if (tid == 0) { info[2 * b] = fixpoint ? (int64_t)reached : -1; info[2 * b + 1] = sweeps; }
}

// the reference's motion order (dijkstra.py:247-260); the first four are straight
__constant__ int kMoves[8][2] = {{1, 0}, {0, 1}, {-1, 0}, {0, -1}, {-1, -1}, {-1, 1}, {1, -1}, {1, 1}};

__global__ void __launch_bounds__(256) path_trace_kernel(const uint32_t *__restrict__ field, int n_fields, int nx, int ny, const int32_t *__restrict__ goals,
                                                         const int64_t *__restrict__ offsets, int64_t n_goals, int32_t *__restrict__ paths,
                                                         unsigned long long *__restrict__ info) {
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= n_goals) return;
    const int f = goals[3 * g];
    int x = goals[3 * g + 1], y = goals[3 * g + 2];
    const int64_t first = offsets[g], slot = offsets[g + 1] - first;
    const uint32_t *F = nullptr;
    uint32_t l = kUnreached;
    if ((unsigned)f < (unsigned)n_fields && (unsigned)x < (unsigned)nx && (unsigned)y < (unsigned)ny) {
        F = field + (int64_t)f * nx * ny;
        l = F[x * ny + y];
    }
    const int64_t len = l == kUnreached ? 0 : (int64_t)(l >> 16) + (int64_t)(l & 0xffffu) + 1;
    if (slot != len) { atomicAdd(info + 1, 1ull); return; }                           // nothing is written for this goal
    if (len == 0) return;
    int32_t *p = paths + 2 * first;
    bool whole = false;
    for (int64_t k = 0; k < len; ++k) {                                               // a + b falls by one per step: at most len cells
        p[2 * k] = x; p[2 * k + 1] = y;
        if (l == 0) { whole = true; break; }
        bool moved = false;
        for (int m = 0; m < 8 && !moved; ++m) {
            const int px = x - kMoves[m][0], py = y - kMoves[m][1];
            if ((unsigned)px >= (unsigned)nx || (unsigned)py >= (unsigned)ny) continue;
            if (m < 4 ? (l >> 16) == 0 : (l & 0xffffu) == 0) continue;
            const uint32_t want = l - (m < 4 ? kStraight : kDiagonal);
            if (F[px * ny + py] == want) { x = px; y = py; l = want; moved = true; }
        }
        if (!moved) break;                                                            // not a field of mnf_path_field
    }
    atomicAdd(info + (whole ? 0 : 1), 1ull);
}

}  // namespace
}  // namespace mnf

using namespace mnf;

extern "C" int64_t mnf_path_field_bytes(int32_t nx, int32_t ny, int32_t n_sources) {
    if (!planner_geometry_ok(nx, ny) || n_sources < 0) return 0;
    return (int64_t)nx * ny * n_sources * (int64_t)sizeof(uint32_t);
}

extern "C" int mnf_path_field(const int32_t *blocked, int32_t n_maps, int32_t nx, int32_t ny, int32_t lim_x, int32_t lim_y, const int32_t *sources,
                              int32_t n_sources, uint32_t *field, int64_t *info, mnf_stream_t stream) {
    MNF_REQUIRE(nx > 0 && ny > 0, "path_field: the map size must be positive (got %d x %d)", nx, ny);
    MNF_REQUIRE(planner_geometry_ok(nx, ny), "path_field: a %d x %d map is more than the %lld bordered cells one workgroup's LDS holds", nx, ny,
                (long long)kMaxBorderedCells);
    MNF_REQUIRE(lim_x >= 0 && lim_x <= nx && lim_y >= 0 && lim_y <= ny, "path_field: limits %d x %d outside [0, %d] x [0, %d]", lim_x, lim_y, nx, ny);
    MNF_REQUIRE(n_sources >= 0, "path_field: n_sources is negative (%d)", n_sources);
    MNF_REQUIRE(n_maps == 1 || n_maps == n_sources, "path_field: n_maps is 1 or n_sources (got %d for %d sources)", n_maps, n_sources);
    MNF_REQUIRE(blocked || n_sources == 0, "path_field: blocked is null");
    MNF_REQUIRE(sources || n_sources == 0, "path_field: sources is null");
    MNF_REQUIRE(field || n_sources == 0, "path_field: field is null");
    MNF_REQUIRE(info || n_sources == 0, "path_field: info is null");
    MNF_REQUIRE(aligned8(info), "path_field: info must be 8-byte aligned");
    if (n_sources == 0) return MNF_OK;
    const int lds = (nx + 2) * (ny + 2) * (int)sizeof(uint32_t);
    MNF_HIP(hipFuncSetAttribute((const void *)path_field_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kMaxBorderedCells * 4));
    hipStream_t s = as_stream(stream);
    ProfScope prof("path_field", s);
    hipLaunchKernelGGL(path_field_kernel, dim3((unsigned)n_sources), dim3(kFieldThreads), lds, s, blocked, n_maps == 1 ? (int64_t)0 : (int64_t)nx * ny, nx, ny,
                       lim_x, lim_y, sources, field, info);
    return launch_status("path_field_kernel");
}

extern "C" int mnf_path_trace(const uint32_t *field, int32_t n_fields, int32_t nx, int32_t ny, const int32_t *goals, const int64_t *offsets, int64_t n_goals,
                              int32_t *paths, int64_t *info, mnf_stream_t stream) {
    MNF_REQUIRE(nx > 0 && ny > 0, "path_trace: the map size must be positive (got %d x %d)", nx, ny);
    MNF_REQUIRE(planner_geometry_ok(nx, ny), "path_trace: a %d x %d map is more than mnf_path_field makes fields of", nx, ny);
    MNF_REQUIRE(n_fields >= 0, "path_trace: n_fields is negative (%d)", n_fields);
    MNF_REQUIRE(n_goals >= 0, "path_trace: n_goals is negative (%lld)", (long long)n_goals);
    MNF_REQUIRE(n_goals <= (int64_t)0x7fffffff * 256, "path_trace: n_goals is more than one launch holds (%lld)", (long long)n_goals);
    MNF_REQUIRE(info, "path_trace: info is null");
    MNF_REQUIRE(aligned8(info), "path_trace: info must be 8-byte aligned");
    MNF_REQUIRE(aligned8(offsets), "path_trace: offsets must be 8-byte aligned");
    MNF_REQUIRE(field || n_fields == 0, "path_trace: field is null");
    MNF_REQUIRE(goals || n_goals == 0, "path_trace: goals is null");
    MNF_REQUIRE(offsets || n_goals == 0, "path_trace: offsets is null");
    MNF_REQUIRE(paths || n_goals == 0, "path_trace: paths is null");
    hipStream_t s = as_stream(stream);
    ProfScope prof("path_trace", s);
    MNF_HIP(hipMemsetAsync(info, 0, 2 * sizeof(int64_t), s));
    if (n_goals == 0) return MNF_OK;
    hipLaunchKernelGGL(path_trace_kernel, dim3((unsigned)ceil_div(n_goals, 256)), dim3(256), 0, s, field, n_fields, nx, ny, goals, offsets, n_goals, paths,
                       reinterpret_cast<unsigned long long *>(info));
    return launch_status("path_trace_kernel");
}
