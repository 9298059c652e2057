// What the map units share (objmap.hip, explore.hip, planning.hip, scanmap.hip): the geometry of a voxel bit grid, the lock-free union-find
// behind both cluster read-outs, the ordered compaction of one workgroup, and the planner's cap.
//
// Bit grid: uint32 bits[planes][wpp]; voxel (x, y, z) of a plane is bit (lin & 31) of word plane * wpp + (lin >> 5), lin = (x * Y + y) * Z + z
// (the estimator's layout); wpp = ceil(X Y Z / 32) rounded up to an even number, so every plane starts 8-byte aligned.  The tail bits of a plane
// are never set by an insert and are masked by every reader (valid_bits).
//
// Union-find over parent[0 .. n), parent[i] = i at the start, shared by every workgroup of a link launch.
//   - Every access of the link launch is an agent-scope relaxed atomic (no L1, coherent across the XCDs); parent[] carries no other data, so
//     nothing needs ordering against it.
//   - unite() hooks the LARGER root under the smaller with a CAS that expects the root to be a root still.  So parent[i] <= i always, every walk
//     strictly descends and ends, and when the launch is over a component's root is its smallest member whatever the schedule: labels taken
//     from roots are the same bytes every time.
//   - A failed CAS means another lane has hooked that root meanwhile; the returned value is an ancestor of it, so the search goes on from there.
//   - find_root() halves the path on its way.  A non-root's parent is only ever replaced by another of its ancestors, and a non-root never
//     becomes a root again, so these plain stores cannot undo a hook.
//   - settled_root() is the read-only walk for the kernels after the link launch, where parent[] no longer changes.
//
// block_rank<kThreads>(keep, &total): the exclusive rank of this thread's `keep` among the workgroup's kThreads threads in thread order (ballot
// rank within the wave, wave totals through LDS), and the workgroup's total, the same value in every thread.  The rank is formed only where
// `keep` is set (0 elsewhere: nobody places a cell that is not kept).  Every thread of the workgroup calls it.  It holds two workgroup barriers,
// one before the wave totals are read and one right after, with nothing but those reads between them, so it can be called once per tile in a
// loop with the running base in a register.
#pragma once
#include "common.h"
#include "reduce_dev.h"

namespace mnf {

// ---------------------------------------------------------------------------------------------------------------- bit grid
constexpr int kMaxAxis = 1 << 24;             // (float)res is exact: an insert compares a floored float against it

struct BitGrid { int X, Y, Z; int64_t n_vox; int64_t wpp; };

// false when the geometry is refused
inline bool make_bit_grid(int32_t planes, int32_t X, int32_t Y, int32_t Z, BitGrid *g) {
    if (planes <= 0 || X <= 0 || Y <= 0 || Z <= 0) return false;
    if (X > kMaxAxis || Y > kMaxAxis || Z > kMaxAxis) return false;
    if ((int64_t)X * Y > (int64_t)1 << 31) return false;
    const int64_t n = (int64_t)X * Y * Z;
    if (n > ((int64_t)1 << 31) - 64) return false;
    const int64_t wpp = (ceil_div(n, 32) + 1) & ~(int64_t)1;
    if (wpp * planes > ((int64_t)1 << 31) - 1) return false;
    *g = {X, Y, Z, n, wpp};
    return true;
}

// the bits of word w of a plane that stand for voxels
__device__ __forceinline__ unsigned int valid_bits(int64_t w, int64_t n_vox) {
    const int64_t left = n_vox - w * 32;
    return left >= 32 ? 0xffffffffu : left <= 0 ? 0u : (1u << (int)left) - 1u;
}

// ---------------------------------------------------------------------------------------------------------------- union-find
__device__ __forceinline__ int load_parent(int *parent, int i) { return __hip_atomic_load(parent + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ int find_root(int *parent, int i) {
    int p = load_parent(parent, i);
    while (p != i) {
        const int gp = load_parent(parent, p);
        if (gp != p) __hip_atomic_store(parent + i, gp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        i = p;
        p = gp;
    }
    return i;
}

__device__ __forceinline__ void unite(int *parent, int a, int b) {
    for (;;) {
        a = find_root(parent, a);
        b = find_root(parent, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }                // a > b
        const int old = atomicCAS(parent + a, a, b);
        if (old == a) return;
        a = old;
    }
}

__device__ __forceinline__ int settled_root(const int *__restrict__ parent, int i) {
    for (int p = parent[i]; p != i; p = parent[i]) i = p;
    return i;
}

// ---------------------------------------------------------------------------------------------------------------- ordered compaction
template <int kThreads>
__device__ __forceinline__ int block_rank(bool keep, int *total) {
    __shared__ int wave_total[kThreads / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long votes = __ballot(keep);
    if (lane == 0) wave_total[wave] = __popcll(votes);
    __syncthreads();
    int n[kThreads / 64];
#pragma unroll
    for (int w = 0; w < kThreads / 64; ++w) n[w] = wave_total[w];
    __syncthreads();                                                 // wave_total is read: the next call may write it
    int all = 0, rank = 0;
#pragma unroll
    for (int w = 0; w < kThreads / 64; ++w) all += n[w];
    if (keep) {                                                      // a wave that keeps nothing skips the sixteen selects
        rank = __popcll(votes & ((1ull << lane) - 1ull));
#pragma unroll
        for (int w = 0; w < kThreads / 64; ++w) rank += w < wave ? n[w] : 0;
    }
    *total = all;
    return rank;
}

// ---------------------------------------------------------------------------------------------------------------- the planner's cap
// (nx + 2)(ny + 2) words of labels with their border are 160 000 B of one workgroup's LDS, and a + b <= nx ny - 1 < 2^16 keeps a label's halves
// apart (planning.hip); the cost map keeps to the same cap, so every map the grid search takes has one (scanmap.hip).
constexpr int64_t kMaxBorderedCells = 40000;
constexpr uint32_t kUnreached = 0xFFFFFFFFu;          // a field's "not reached"

inline bool planner_geometry_ok(int32_t nx, int32_t ny) { return nx > 0 && ny > 0 && ((int64_t)nx + 2) * ((int64_t)ny + 2) <= kMaxBorderedCells; }

}  // namespace mnf
