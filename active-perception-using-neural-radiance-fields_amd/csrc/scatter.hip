// The hash-table half of the field's backward (train.hip runs the matrix-core half): the trilinear scatter of dL/d(hash features), which dgrad_kernel
// leaves level-major in the train workspace, into the dense fp32 table gradient.  Nothing here touches a matrix-core operand, so the unit is
// compiled once and serves handles of both operand types.  Host interface: scatter.h.
#include <cstring>

#include "field_dev.h"
#include "scatter.h"

namespace mnf {
// field_dev.h keeps its helpers in the per-type namespace; the ones used here (count_here, chunk_tiles, hash_prep, kWaveSamples) do not depend on the type
using namespace f16;

// ------------------------------------------------------------------ hash-grid gradient scatter
// Deterministic mode (mnf_train_opts.deterministic): the table gradient is accumulated in 64-bit fixed point (value * 2^56, integer
// atomics: associative, so the result does not depend on the order in which the adds arrive), then converted to fp32 once.  The
// memory-side atomic unit takes 8-byte integer adds at the request rate of 4-byte float adds (tools/atomic_bench.hip), so the mode
// costs the wider zero-fill and the conversion pass, not scatter time.  Range +-128 (saturating), resolution 1.4e-17.
constexpr float kFixScale = 72057594037927936.0f;        // 2^56
constexpr double kFixInv = 1.0 / 72057594037927936.0;
__device__ __forceinline__ unsigned long long to_fixed(float v) {
    const float c = fminf(fmaxf(v, -127.99999f), 127.99999f);
    return (unsigned long long)__float2ll_rn(c * kFixScale);              // NaN -> 0 (llrint of NaN is unspecified: guard below)
}

struct HashBwdArgs {
    const float *positions;   // aabb-normalised positions xn = (x - aabb_min) / (aabb_max - aabb_min) [N,3] (normalize_kernel): the
                              // three divisions are done once per sample, not once per sample, level and lane
    const float *dX;      // [16][Np][4]
    int64_t Np;
    int chunk, n_chunks;  // this launch covers tile range `chunk` of `n_chunks` (chunk_tiles)
    int level0;           // first level of this launch (experiments; 0 in production)
    int n_walk_levels;    // levels level0 .. level0 + n_walk_levels - 1
    float *repl;          // [kReplicas][repl_floats]: private copies of the coarsest levels' gradient (see below)
    uint32_t repl_floats;
    int repl_levels;
    float *g_table;       // fp32 [entries][4]
    int64_t n;
    const int64_t *n_dev;
    unsigned long long *flush_count;   // diagnostic build (MNF_SCATTER_COUNT=1): quad atomics issued per level, else NULL
    unsigned long long *q_table, *q_repl;   // deterministic mode: fixed-point table gradient [entries][4] and replicas, else NULL
    unsigned long long *q_bad;              // deterministic mode: number of non-finite contributions (they cannot be represented in fixed point)
    float aabb[6];
    LevelMeta levels[16];
};

// ngp.py:177-178 once per sample for the scatter below (the same expression as the forward kernel's fetch_sample)
__global__ void __launch_bounds__(256) normalize_kernel(const float *__restrict__ pos, int64_t n_cap, const int64_t *n_dev, float a0, float a1, float a2,
                                                        float a3, float a4, float a5, float *__restrict__ xn) {
    const float lo[3] = {a0, a1, a2}, hi[3] = {a3, a4, a5};
    const int64_t n = count_here(n_cap, n_dev);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < 3 * n; i += (int64_t)blockDim.x * gridDim.x) {
        const int d = (int)(i % 3);
        xn[i] = (pos[i] - lo[d]) / (hi[d] - lo[d]);
    }
}

// Samples arrive sorted by ray and by distance along the ray, so consecutive samples usually sit in the same grid cell
// of a level (always at the coarse levels, often at the fine ones).  A scattered float atomic is the slow operation
// here (MI355X: ~17x below the contiguous rate) and the kernel is bound by the rate of memory-side read-modify-writes,
// so everything below is about issuing fewer of them.  (History: one atomic per lane and corner 94 ms; runs of lanes in
// one cell summed by a segmented lane scan, tails only 21 ms; LDS transpose to 16-byte quad atomics 3.7 ms; the walk
// below with face sharing 3.4 ms.)
// The coarsest dense levels have a few thousand entries that every ray of a camera crosses near its origin: their
// atomics pile up on the same addresses (level 0 alone cost as much as the finest level).  Workgroups therefore add
// into one of kReplicas private copies of those levels, which a small kernel folds into the gradient afterwards.
constexpr int kReplicas = 16;
constexpr uint32_t kReplMaxEntries = 131072;

__global__ void __launch_bounds__(256) fold_replicas_fixed_kernel(const unsigned long long *__restrict__ repl, uint32_t repl_floats,
                                                                  unsigned long long *__restrict__ q_table) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= repl_floats) return;
    unsigned long long acc = 0;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc += repl[(size_t)r * repl_floats + i];
    if (acc) q_table[i] += acc;
}

// fixed point -> fp32 gradient (overwrites the table part of the gradient vector)
__global__ void __launch_bounds__(256) fixed_to_float_kernel(const long long *__restrict__ q, float *__restrict__ g, int64_t n,
                                                             const unsigned long long *__restrict__ bad) {
    const bool poisoned = *bad != 0;     // a non-finite contribution was met: the gradient says so (the NaN guard of pipeline.py:520-529 sees it)
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)blockDim.x * gridDim.x)
        g[i] = poisoned && i == 0 ? __builtin_nanf("") : (float)((double)q[i] * kFixInv);
}

__global__ void __launch_bounds__(256) fold_replicas_kernel(const float *__restrict__ repl, uint32_t repl_floats, float *__restrict__ g_table) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= repl_floats) return;
    float acc = 0.f;
#pragma unroll
    for (int r = 0; r < kReplicas; ++r) acc += repl[(size_t)r * repl_floats + i];
    if (acc != 0.f) g_table[i] += acc;
}

// The scatter as a WALK along the sample order.  A half-wave owns a chunk of kWalkChunk consecutive samples of one level;
// its 32 lanes are the 8 corners x 4 features of a grid cell.  Samples are visited in order, every lane accumulating
// w_corner * g_feature for the open cell in a register; when the cell changes the sums go out as quad-atomics (the four
// features of a corner are 16 contiguous bytes).  What the lane-scan form cannot do: when the ray steps into a FACE
// neighbour, the four corners on the shared face stay in registers (they move to the partner lanes, lane ^ 4 / 8 / 16)
// and only the four corners left behind are flushed; edge and vertex neighbours are reached by two or three such
// crossings (6 or 7 flushed corners instead of 8).  The kernel is bound by the rate of memory-side read-modify-writes.  Ray structure is not needed: runs are found by comparing
// consecutive cells, and a chunk boundary only costs one extra flush.
constexpr int kWalkChunk = 128;

template <bool DET>
__global__ void __launch_bounds__(256) hash_bwd_walk_kernel(const HashBwdArgs args) {
    const int sub = threadIdx.x & 31;                 // lane inside the half-wave
    const int corner = sub >> 2, feat = sub & 3;
    const int bx = corner & 1, by = (corner >> 1) & 1, bz = corner >> 2;
    const int64_t n_cnt = count_here(args.n, args.n_dev);
    int64_t rt0, rt1;
    chunk_tiles(n_cnt, args.chunk, args.n_chunks, rt0, rt1);
    const int64_t s_lo = rt0 * kWaveSamples, n_all = rt1 * kWaveSamples < n_cnt ? rt1 * kWaveSamples : n_cnt;       // samples [s_lo, n_all) of this launch
    // A bounded number of workgroups walks all (level, chunk) pairs (level by level, so that the workgroups of the moment add into the same few
    // megabytes): the kernel is bound by the atomic unit, not by waves in flight, and the wave slots it leaves are what lets the binned passes
    // and the weight gradients run beside it instead of behind it.
    const int64_t chunks = n_all > s_lo ? (n_all - s_lo + kWalkChunk - 1) / kWalkChunk : 0;
    const int64_t items = chunks * args.n_walk_levels;
    for (int64_t item = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 5; item < items; item += ((int64_t)gridDim.x * blockDim.x) >> 5) {
    const int64_t chunk = item % chunks;
    const int l = (int)(item / chunks) + args.level0;
    const int64_t i0 = s_lo + chunk * kWalkChunk;
    const int64_t i1 = i0 + kWalkChunk < n_all ? i0 + kWalkChunk : n_all;
    const LevelMeta m = args.levels[l];
    const uint32_t replica = (uint32_t)((chunk >> 3) % kReplicas);
    float *const g_dst = l < args.repl_levels ? args.repl + (size_t)replica * args.repl_floats : args.g_table;
    unsigned long long *const q_dst = !DET ? nullptr : (l < args.repl_levels ? args.q_repl + (size_t)replica * args.repl_floats : args.q_table);
    const float *gl = args.dX + ((int64_t)l * args.Np) * 4 + feat;

    float acc = 0.0f;
    bool open = false;
    int cx = 0, cy = 0, cz = 0;                       // cell of the open run
    auto flush = [&]() {                              // this lane's corner of the open cell
        if (acc != 0.0f) {
            const uint32_t px = (uint32_t)cx + bx, py = (uint32_t)cy + by, pz = (uint32_t)cz + bz;
            uint32_t idx;
            if (m.hashed) {
                idx = (px ^ (py * 2654435761u) ^ (pz * 805459861u)) & (m.size - 1u);
            } else {
                idx = px + py * m.res + pz * m.res * m.res;
                uint32_t q = __umulhi(m.div_magic, idx);
                q = (((idx - q) >> 1) + q) >> m.div_shift;
                idx -= q * m.size;
            }
#ifdef MNF_DIAG
            if (args.flush_count && feat == 0) atomicAdd(&args.flush_count[l], 1ull);
#endif
            if (DET) {
                // a contribution outside the fixed-point range would saturate silently into a wrong finite gradient: it poisons the
                // step like a non-finite one
                if (fabsf(acc) < 127.99999f) atomicAdd(q_dst + ((size_t)(m.offset + idx) << 2) + feat, to_fixed(acc));
                else atomicAdd(args.q_bad, 1ull);          // too large / NaN / Inf: reported through the converted gradient (fixed_to_float_kernel)
            }
            else atomicAdd(g_dst + ((size_t)(m.offset + idx) << 2) + feat, acc);
        }
        acc = 0.0f;
    };
    constexpr int B = 8;                              // samples fetched ahead of the sequential part
    for (int64_t i = i0; i < i1; i += B) {
        float sx[B], sy[B], sz[B], g[B];
#pragma unroll
        for (int b = 0; b < B; ++b) {
            const int64_t k = i + b < i1 ? i + b : i1 - 1;
            sx[b] = args.positions[3 * k]; sy[b] = args.positions[3 * k + 1]; sz[b] = args.positions[3 * k + 2];
            g[b] = gl[k * 4];
        }
#pragma unroll
        for (int b = 0; b < B; ++b) {
            if (i + b >= i1) break;
            // position -> cell and fractions, exactly as hash_prep
            const float x0 = __builtin_fmaf(m.scale, sx[b], 0.5f);
            const float x1 = __builtin_fmaf(m.scale, sy[b], 0.5f);
            const float x2 = __builtin_fmaf(m.scale, sz[b], 0.5f);
            const float f0 = floorf(x0), f1 = floorf(x1), f2 = floorf(x2);
            const int c0 = (int)f0, c1 = (int)f1, c2 = (int)f2;
            const int dx = c0 - cx, dy = c1 - cy, dz = c2 - cz;
            if (!open) {
                open = true;
                cx = c0; cy = c1; cz = c2;
            } else if ((dx | dy | dz) != 0) {         // half-wave uniform
                const int ax = dx < 0 ? -dx : dx, ay = dy < 0 ? -dy : dy, az = dz < 0 ? -dz : dz;
                if ((ax | ay | az) > 1) {
                    flush();                           // a jump (new ray, or a step longer than a cell)
                    cx = c0; cy = c1; cz = c2;
                } else {
                    // one face crossing per changed axis, through the intermediate cells: the corners on the far side of
                    // the cell being left are the near side of the next one and stay in registers (partner lane)
                    auto face_move = [&](int bit, int dir, int mask) {
                        const bool stays_behind = dir > 0 ? bit == 0 : bit == 1;
                        if (stays_behind) flush();
                        const float moved = __shfl_xor(acc, mask, 64);
                        acc = stays_behind ? moved : 0.0f;
                    };
                    if (dx) { face_move(bx, dx, 4); cx = c0; }
                    if (dy) { face_move(by, dy, 8); cy = c1; }
                    if (dz) { face_move(bz, dz, 16); cz = c2; }
                }
            }
            const float fx = x0 - f0, fy = x1 - f1, fz = x2 - f2;
            const float wx = bx ? fx : 1.0f - fx, wy = by ? fy : 1.0f - fy, wz = bz ? fz : 1.0f - fz;
            acc += (((1.0f * wx) * wy) * wz) * g[b];
        }
    }
    flush();
    }
}

// ---- the large hashed levels: binned scatter -------------------------------------------------------------------------------------
// The walk above is bound by the memory-side atomic unit (~21 G 64-byte requests/s whatever they carry, profiles/r03_atomic_microbench.txt),
// and on the fine levels nearly every corner of every sample is a request of its own (hashed neighbours are not neighbours in memory).
// Those levels go through memory instead: a level's table (2^k entries) is cut into bins of kBinEntries consecutive entries whose fp32
// gradient fits in LDS.  Pass A (bin_items_kernel) writes one 16-byte item per (sample, corner) — the four feature gradients with the entry's
// index inside its bin kept in their lowest mantissa bits — to the bin's list (slots reserved per workgroup: one returning atomic per bin
// and workgroup).  Pass B (bin_accumulate_kernel), one workgroup per (level, bin), streams its list, adds into LDS and adds
// the bin's sums to the gradient with plain 16-byte read-modify-writes: it is the only writer of those entries at that time.  The LDS sums
// are DOUBLES: ds_add_f32 retires about one lane every 2.5 clocks per CU (4 x slower than the loads feed it), ds_add_f64 and the integer
// adds run at the rate of the loads (tools/bin_bench.hip, profiles/r03_bin_bench.txt).  A list that
// is full sends its items to the gradient with float atomics as before, so the bins only need to be sized for a uniform hash.
constexpr int kBinEntriesLog2 = 12;
constexpr uint32_t kBinEntries = 1u << kBinEntriesLog2;     // x 4 features x 8 bytes = 128 KB of LDS per workgroup of pass B
constexpr int kMaxBins = 512;                                // per level: tables up to 2^21 entries
constexpr int kBinThreadsB = 1024;
static_assert(16 * kMaxBins == kScatterCursors, "scatter.h: the cursors the caller clears");

struct BinArgs {
    const float *positions;   // normalised positions [N,3]
    const float *dX;          // [16][Np][4]
    int64_t Np, n;
    const int64_t *n_dev;
    int chunk, n_chunks;      // pass A of this launch covers tile range `chunk` of `n_chunks` (chunk_tiles); pass B runs once, behind the last pass A
    int level0, n_levels;     // levels level0 .. level0 + n_levels - 1, all hashed with size a multiple of kBinEntries
    float4 *items;            // [n_levels][bins of that level][cap]: level k's lists start at item_base[k]
    uint32_t *cursors;        // [n_levels][kMaxBins] items handed out per list (may exceed cap: the excess went to the atomics)
    uint32_t cap;             // items per list
    float *g_table;           // fp32 [entries][4]
    LevelMeta levels[16];
};

// index bits into / out of the lowest 3 mantissa bits of each of the four values (round to nearest on the remaining 20 bits; a non-finite
// value stays non-finite, so the NaN guard of the step still sees it)
__device__ __forceinline__ float4 pack_item(const float v[4], uint32_t idx) {
    float4 o;
    float *po = &o.x;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        uint32_t b = __builtin_bit_cast(uint32_t, v[k]);
        if ((b & 0x7f800000u) != 0x7f800000u) b += 4u;          // (Inf / NaN: no carry out of the exponent)
        b = (b & ~7u) | ((idx >> (3 * k)) & 7u);
        po[k] = __builtin_bit_cast(float, b);
    }
    return o;
}

static_assert(kBinEntriesLog2 <= 12, "pack_item keeps 3 index bits per value");

constexpr int kBinChunk = 2;                                 // sub-chunks of 256 samples per workgroup of pass A
constexpr int kBinStage = kBinChunk * 256 * 8;               // items staged in LDS per workgroup (64 KB)

__global__ void __launch_bounds__(256) bin_items_kernel(const BinArgs args) {
    __shared__ uint32_t s_cnt[kMaxBins], s_off[kMaxBins];
    __shared__ float4 s_stage[kBinStage];
    __shared__ uint16_t s_binof[kBinStage];
    __shared__ uint32_t s_total;
    // level fastest: neighbouring workgroups reserve in different levels' cursors
    const int lk = (int)(blockIdx.x % (unsigned)args.n_levels), l = lk + args.level0;
    const int64_t chunk = blockIdx.x / (unsigned)args.n_levels;
    const LevelMeta m = args.levels[l];
    const uint32_t nb = m.size >> kBinEntriesLog2;
    const int64_t n_cnt = count_here(args.n, args.n_dev);
    int64_t rt0, rt1;
    chunk_tiles(n_cnt, args.chunk, args.n_chunks, rt0, rt1);
    const int64_t n_all = rt1 * kWaveSamples < n_cnt ? rt1 * kWaveSamples : n_cnt;
    const int64_t first = rt0 * kWaveSamples + chunk * (kBinChunk * 256);
    if (first >= n_all) return;
    for (uint32_t b = threadIdx.x; b < nb; b += 256) s_cnt[b] = 0;
    __syncthreads();
    // 1. this thread's samples: entries, blend weights, gradient; rank of every item among the workgroup's items of its list
    uint32_t idx[kBinChunk][8], rank[kBinChunk][8];
    float w[kBinChunk][8];
    float4 g[kBinChunk];
#pragma unroll
    for (int sc = 0; sc < kBinChunk; ++sc) {
        const int64_t i = first + sc * 256 + threadIdx.x;
        if (i < n_all) {
            float xn[3];
#pragma unroll
            for (int d = 0; d < 3; ++d) xn[d] = args.positions[3 * i + d];
            LevelPrep p;
            hash_prep(m, xn, p);
            g[sc] = reinterpret_cast<const float4 *>(args.dX)[(int64_t)l * args.Np + i];
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                idx[sc][c] = p.off[c] >> 3;                          // entry inside the level
                w[sc][c] = ((c & 1) ? p.wxy[(c >> 1) & 1].y : p.wxy[(c >> 1) & 1].x) * p.wz[c >> 2];
                rank[sc][c] = atomicAdd(&s_cnt[idx[sc][c] >> kBinEntriesLog2], 1u);
            }
        }
    }
    __syncthreads();
    // 2. where each list's run starts in the staging buffer (exclusive scan, one wave) ...
    if (threadIdx.x < 64) {
        uint32_t run = 0;
        for (uint32_t b0 = 0; b0 < nb; b0 += 64) {
            const uint32_t b = b0 + threadIdx.x;
            const uint32_t c = b < nb ? s_cnt[b] : 0u;
            uint32_t incl = c;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const uint32_t t = __shfl_up(incl, d, 64);
                if ((int)threadIdx.x >= d) incl += t;
            }
            if (b < nb) s_off[b] = run + incl - c;
            run += __shfl(incl, 63, 64);
        }
        if (threadIdx.x == 0) s_total = run;
    }
    __syncthreads();
    // ... and in the list itself: one returning add per list and workgroup; s_cnt becomes (slot in the list) - (position in the staging buffer)
    for (uint32_t b = threadIdx.x; b < nb; b += 256) {
        const uint32_t c = s_cnt[b];
        const uint32_t base = c ? atomicAdd(&args.cursors[(size_t)lk * kMaxBins + b], c) : 0u;
        s_cnt[b] = base - s_off[b];
    }
    // 3. items into the staging buffer, list by list
#pragma unroll
    for (int sc = 0; sc < kBinChunk; ++sc) {
        const int64_t i = first + sc * 256 + threadIdx.x;
        if (i < n_all) {
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const uint32_t b = idx[sc][c] >> kBinEntriesLog2, pos = s_off[b] + rank[sc][c];
                const float v[4] = {w[sc][c] * g[sc].x, w[sc][c] * g[sc].y, w[sc][c] * g[sc].z, w[sc][c] * g[sc].w};
                s_stage[pos] = pack_item(v, idx[sc][c] & (kBinEntries - 1u));
                s_binof[pos] = (uint16_t)b;
            }
        }
    }
    __syncthreads();
    // 4. out: consecutive lanes write consecutive slots of a list
    float4 *const lists = args.items + (size_t)lk * nb * args.cap;      // every binned level has the same size (2^k, checked by the host)
    const uint32_t total = s_total;
    for (uint32_t p = threadIdx.x; p < total; p += 256) {
        const uint32_t b = s_binof[p], slot = s_cnt[b] + p;
        const float4 it = s_stage[p];
        if (slot < args.cap) {
            lists[(size_t)b * args.cap + slot] = it;
        } else {                                                 // the list is full: straight to the gradient
            const uint32_t bits[4] = {__float_as_uint(it.x), __float_as_uint(it.y), __float_as_uint(it.z), __float_as_uint(it.w)};
            const uint32_t e = (bits[0] & 7u) | ((bits[1] & 7u) << 3) | ((bits[2] & 7u) << 6) | ((bits[3] & 7u) << 9);
            float *dst = args.g_table + ((size_t)(m.offset + b * kBinEntries + e) << 2);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float v = __uint_as_float(bits[k] & ~7u);
                if (v != 0.f) atomicAdd(dst + k, v);
            }
        }
    }
}

__global__ void __launch_bounds__(kBinThreadsB) bin_accumulate_kernel(const BinArgs args) {
    __shared__ double s_sum[kBinEntries * 4];
    const int lk = blockIdx.y, l = lk + args.level0;
    const LevelMeta m = args.levels[l];
    const uint32_t nb = m.size >> kBinEntriesLog2, b = blockIdx.x;
    if (b >= nb) return;
    uint32_t count = args.cursors[(size_t)lk * kMaxBins + b];
    if (count == 0) return;
    if (count > args.cap) count = args.cap;
    for (uint32_t e = threadIdx.x; e < kBinEntries * 4; e += kBinThreadsB) s_sum[e] = 0.0;
    __syncthreads();
    const float4 *list = args.items + ((size_t)lk * nb + b) * args.cap;
    constexpr int U = 4;                                         // items in flight per lane
    for (uint32_t i0 = threadIdx.x; i0 < count; i0 += kBinThreadsB * U) {
        typedef float v4f __attribute__((ext_vector_type(4)));
        v4f it[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t i = i0 + u * kBinThreadsB;
            it[u] = reinterpret_cast<const v4f *>(list)[i < count ? i : count - 1u];
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (i0 + u * kBinThreadsB >= count) break;
            const float f0 = it[u][0], f1 = it[u][1], f2 = it[u][2], f3 = it[u][3];     // (__builtin_bit_cast straight from a vector element reads element 0)
            const uint32_t b0 = __float_as_uint(f0), b1 = __float_as_uint(f1), b2 = __float_as_uint(f2), b3 = __float_as_uint(f3);
            const uint32_t e = (b0 & 7u) | ((b1 & 7u) << 3) | ((b2 & 7u) << 6) | ((b3 & 7u) << 9);
            double *dst = s_sum + e * 4;
            atomicAdd(dst, (double)__uint_as_float(b0 & ~7u));
            atomicAdd(dst + 1, (double)__uint_as_float(b1 & ~7u));
            atomicAdd(dst + 2, (double)__uint_as_float(b2 & ~7u));
            atomicAdd(dst + 3, (double)__uint_as_float(b3 & ~7u));
        }
    }
    __syncthreads();
    // this bin's sums into the gradient: plain read-modify-writes (nothing else touches these entries at this time)
    float *const out = args.g_table + (((size_t)m.offset + (size_t)b * kBinEntries) << 2);
    for (uint32_t i = threadIdx.x; i < kBinEntries * 4; i += kBinThreadsB) {
        const float a = (float)s_sum[i];
        if (a != 0.f) {
            out[i] += a;
        }
    }
}

// Reference form of the scatter (MNF_HASH_BWD_SIMPLE=1, debugging and A/B timing): one lane per sample, one atomic per
// corner and feature, no run merging.
__global__ void __launch_bounds__(256) hash_bwd_simple_kernel(const HashBwdArgs args) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count_here(args.n, args.n_dev)) return;
    float xn[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) xn[d] = args.positions[3 * i + d];
    const int l = blockIdx.y + args.level0;
    const LevelMeta m = args.levels[l];
    float *const g_dst = l < args.repl_levels ? args.repl + (size_t)(blockIdx.x % kReplicas) * args.repl_floats : args.g_table;
    LevelPrep p;
    hash_prep(m, xn, p);
    const float4 g = reinterpret_cast<const float4 *>(args.dX)[(int64_t)l * args.Np + i];
#pragma unroll
    for (int corner = 0; corner < 8; ++corner) {
        const float w = ((corner & 1) ? p.wxy[(corner >> 1) & 1].y : p.wxy[(corner >> 1) & 1].x) * p.wz[corner >> 2];
        float *dst = g_dst + (size_t)p.base * 4 + (p.off[corner] >> 1);   // byte offset of the fp16 entry / 2 == float index inside the level
        const float v[4] = {w * g.x, w * g.y, w * g.z, w * g.w};
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (v[k] != 0.f) atomicAdd(dst + k, v[k]);
    }
}

// the binned scatter's plan for an upper bound of n samples: levels [first, 16) (all hashed, one size, whole bins), lists per level, items per list
constexpr int kBinLevel0Default = 12;      // measured: round 3 (tools/r03_bins_step.sh, profiles/r03_bins_step_*.txt) the step time was flat from 10 to 12, worse below and above (11 then);
                                           // round 4, with wgrad's lighter traffic, 12 is 60 us ahead of 11 at 1.0 M samples (3.393 -> 3.327 ms, four alternations on one box) and equal at 0.25 M
static void bin_plan(const mnf_field_s *f, int64_t n, int want, int &first_binned, uint32_t &nb, uint32_t &cap) {
    first_binned = 16; nb = 0; cap = 0;
    if (n < 8192) return;                    // small batches: the walk alone (pass B costs ~20 us whatever it is given)
    for (int l = 15; l >= want && l >= 0; --l) {
        const LevelMeta &lm = f->levels[l];
        if (!lm.hashed || lm.size < kBinEntries || (lm.size & (lm.size - 1u)) || lm.size != f->levels[15].size || (lm.size >> kBinEntriesLog2) > (uint32_t)kMaxBins) break;
        first_binned = l;
    }
    if (first_binned == 16) return;
    nb = f->levels[15].size >> kBinEntriesLog2;
    const uint64_t per_list = (uint64_t)n * 8 / nb;
    cap = (uint32_t)(per_list + per_list / 8 + 2048);      // a uniform hash fills the lists evenly; the excess of a full one goes to the atomics
}

// the leading dense levels while they stay small: they are scattered into kReplicas private copies
static int replicated_levels(const mnf_field_s *f, uint32_t &entries) {
    int l = 0;
    for (entries = 0; l < 16 && !f->levels[l].hashed && f->levels[l].offset == entries && entries + f->levels[l].size <= kReplMaxEntries; ++l) entries += f->levels[l].size;
    return l;
}

ScatterWorkspace scatter_workspace(const mnf_field_s *f, int64_t n) {
    int first; uint32_t nb, cap;
    bin_plan(f, n, kBinLevel0Default, first, nb, cap);
    return {(size_t)kReplicas * kReplMaxEntries * 4 * sizeof(float), (size_t)(16 - first) * nb * cap};
}

void scatter_normalize(const mnf_field_s *f, const float *positions, int64_t n, const int64_t *n_dev, float *xn, hipStream_t stream) {
    const float *ab = f->cfg.aabb;
    const int64_t blocks = ceil_div(3 * n, 256);
    hipLaunchKernelGGL(normalize_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, stream, positions, n, n_dev, ab[0], ab[1], ab[2],
                       ab[3], ab[4], ab[5], xn);
}

int scatter_begin(const mnf_field_s *f, float *repl, bool deterministic, hipStream_t side) {
    uint32_t repl_entries;
    if (replicated_levels(f, repl_entries) && !deterministic) MNF_HIP(hipMemsetAsync(repl, 0, (size_t)kReplicas * repl_entries * 4 * sizeof(float), side));
    return MNF_OK;
}

int scatter_run(const ScatterCall &c) {
    const mnf_field_s *f = c.f;
    const int64_t n = c.n;
    const int n_chunks = c.n_chunks;
    const bool deterministic = c.deterministic;
    hipStream_t ss = c.side;
    HashBwdArgs hb = {};      // (level0 = chunk = 0, no flush counter, no fixed-point buffers)
    hb.positions = c.xn; hb.dX = c.dX; hb.Np = c.Np; hb.g_table = c.g_table; hb.n = n; hb.n_dev = c.n_dev;
    std::memcpy(hb.aabb, f->cfg.aabb, sizeof(hb.aabb));
    std::memcpy(hb.levels, f->levels, sizeof(hb.levels));
    int n_levels = 16;
    hb.n_chunks = 1;
    if (const char *e = diag_env("MNF_HASH_BWD_LEVELS")) { int lo = 0, hi = 16; if (sscanf(e, "%d,%d", &lo, &hi) == 2) { hb.level0 = lo; n_levels = hi - lo; } }
    // replicated coarse levels (their own region of the workspace, zeroed by scatter_begin)
    uint32_t repl_entries;
    hb.repl_levels = replicated_levels(f, repl_entries);
    hb.repl_floats = repl_entries * 4;
    hb.repl = c.repl;
    const size_t q_table_words = (size_t)f->table_entries * 4, q_repl_words = (size_t)kReplicas * kReplMaxEntries * 4;
    if (deterministic) {
        if (!*c.d_qtable) MNF_HIP(hipMalloc((void **)c.d_qtable, (q_table_words + q_repl_words + 8) * sizeof(unsigned long long)));
        hb.q_table = *c.d_qtable; hb.q_repl = hb.q_table + q_table_words; hb.q_bad = hb.q_repl + q_repl_words;
    }
#ifdef MNF_DIAG
    static unsigned long long *d_flush = nullptr;
    if (diag_env("MNF_SCATTER_COUNT")) {
        if (!d_flush) MNF_HIP(hipMalloc((void **)&d_flush, 16 * sizeof(unsigned long long)));
        MNF_HIP(hipMemsetAsync(d_flush, 0, 16 * sizeof(unsigned long long), ss));
        hb.flush_count = d_flush;
    }
#endif
    static const bool simple = diag_env("MNF_HASH_BWD_SIMPLE") != nullptr;   // debugging aid: one atomic per lane, corner and feature
    // levels [first_binned, 16): through the bins (all of them hashed tables of one size that whole bins tile); the rest: the walk
    int first_binned = 16;
    uint32_t nb_plan = 0, cap = 0;
    if (!deterministic && !simple && n_levels == 16) {
        int want = kBinLevel0Default;
        if (const char *e = diag_env("MNF_BIN_LEVEL0")) want = atoi(e);
        bin_plan(f, n, want, first_binned, nb_plan, cap);
        if (const char *e = diag_env("MNF_BIN_CAP")) cap = (uint32_t)atoi(e);     // tests: force the full-list path
        while (first_binned < 16 && (size_t)(16 - first_binned) * nb_plan * cap > c.bin_items_n) ++first_binned;      // (a diagnostic plan larger than the workspace's)
    }
    BinArgs ba;
    const int n_binned = 16 - first_binned;
    if (n_binned > 0) {
        ba.positions = hb.positions; ba.dX = hb.dX; ba.Np = hb.Np; ba.n = n; ba.n_dev = c.n_dev; ba.level0 = first_binned; ba.n_levels = n_binned;
        ba.items = c.bin_items; ba.cursors = c.d_bin_cursors; ba.cap = cap; ba.g_table = hb.g_table;
        std::memcpy(ba.levels, f->levels, sizeof(ba.levels));
        n_levels = first_binned;
    }
    MNF_HIP(hipStreamWaitEvent(ss, c.ev_chunk[0], 0));
    const int prof_scatter = prof_start("hash_scatter", ss);
    hb.n_walk_levels = n_levels;
    int walk_wgs = 8;                                                                   // workgroups per CU of the 256 (gfx950 only: as the field kernel)
    if (const char *e = diag_env("MNF_WALK_WGS")) walk_wgs = atoi(e);
    const int64_t range_samples = (ceil_div(ceil_div(n, kWaveSamples), n_chunks) + 1) * kWaveSamples;      // samples of one range of dgrad's tiles, at most
    const int64_t walk_full = ceil_div(ceil_div(range_samples, kWalkChunk) * 32, 256) * (n_levels > 0 ? n_levels : 1);
    const dim3 walk_grid((unsigned)(walk_wgs > 0 && walk_full > (int64_t)256 * walk_wgs ? (int64_t)256 * walk_wgs : (walk_full > 0 ? walk_full : 1)));
    if (deterministic) {
        MNF_HIP(hipStreamWaitEvent(ss, c.ev_chunk[0], 0));
        MNF_HIP(hipMemsetAsync(hb.q_table, 0, q_table_words * sizeof(unsigned long long), ss));
        if (hb.repl_levels) MNF_HIP(hipMemsetAsync(hb.q_repl, 0, (size_t)kReplicas * hb.repl_floats * sizeof(unsigned long long), ss));
        MNF_HIP(hipMemsetAsync(hb.q_bad, 0, sizeof(unsigned long long), ss));
        hipLaunchKernelGGL(hash_bwd_walk_kernel<true>, walk_grid, dim3(256), 0, ss, hb);
        if (hb.repl_levels)
            hipLaunchKernelGGL(fold_replicas_fixed_kernel, dim3((hb.repl_floats + 255) / 256), dim3(256), 0, ss, (const unsigned long long *)hb.q_repl,
                               hb.repl_floats, hb.q_table);
        hipLaunchKernelGGL(fixed_to_float_kernel, dim3(4096), dim3(256), 0, ss, reinterpret_cast<const long long *>(hb.q_table), hb.g_table,
                           (int64_t)q_table_words, (const unsigned long long *)hb.q_bad);
    } else {
        if (n_binned > 0) {
            const uint32_t nb = f->levels[15].size >> kBinEntriesLog2;
            static const bool same_stream = diag_env("MNF_BIN_SAME_STREAM") != nullptr;     // timing experiments: bins in front of the walk on one stream
            hipStream_t s2 = same_stream ? ss : c.side2;
            MNF_HIP(hipStreamWaitEvent(s2, c.ev_chunk[0], 0));
            const int prof_bins = prof_start("hash_scatter_bins", s2);
            // (list cursors: zeroed by the caller, scatter.h)
            // (Measured and dropped, tools/r03_walk_wgs.sh: pass B level by level or half by half on a fourth stream under the next pass A — 5.8 and 5.6 ms
            // per step against 5.55-5.6 for one launch each: walk, bins and wgrad together are bound by HBM, the order inside does not matter.)
            for (int k = 0; k < n_chunks; ++k) {          // pass A range by range, each behind its dgrad; pass B once, behind the last
                if (k) MNF_HIP(hipStreamWaitEvent(s2, c.ev_chunk[k], 0));
                ba.chunk = k; ba.n_chunks = n_chunks;
                hipLaunchKernelGGL(bin_items_kernel, dim3((unsigned)(ceil_div(range_samples, kBinChunk * 256) * n_binned)), dim3(256), 0, s2, ba);
            }
            hipLaunchKernelGGL(bin_accumulate_kernel, dim3(nb, n_binned), dim3(kBinThreadsB), 0, s2, ba);
            prof_stop(prof_bins, s2);
            MNF_HIP(hipEventRecord(c.ev_join2, s2));
            MNF_HIP(hipStreamWaitEvent(c.stream, c.ev_join2, 0));
        }
        if (simple) {
            MNF_HIP(hipStreamWaitEvent(ss, c.ev_chunk[n_chunks - 1], 0));
            hipLaunchKernelGGL(hash_bwd_simple_kernel, dim3((unsigned)ceil_div(n, 256), n_levels), dim3(256), 0, ss, hb);
        } else {
            for (int k = 0; k < n_chunks; ++k) {
                MNF_HIP(hipStreamWaitEvent(ss, c.ev_chunk[k], 0));
                hb.chunk = k; hb.n_chunks = n_chunks;
                if (n_levels > 0) hipLaunchKernelGGL(hash_bwd_walk_kernel<false>, walk_grid, dim3(256), 0, ss, hb);
            }
        }
        if (hb.repl_levels)
            hipLaunchKernelGGL(fold_replicas_kernel, dim3((hb.repl_floats + 255) / 256), dim3(256), 0, ss, hb.repl, hb.repl_floats, hb.g_table);
    }
    int rc = launch_status("hash_bwd_walk_kernel");
    if (rc) return rc;
    prof_stop(prof_scatter, ss);
    rc = launch_status("fold_replicas_kernel");
#ifdef MNF_DIAG
    if (hb.flush_count) {      // quad atomics per level of this backward (synchronises: diagnostic only)
        unsigned long long h[16];
        MNF_HIP(hipMemcpyAsync(h, hb.flush_count, sizeof(h), hipMemcpyDeviceToHost, ss));
        MNF_HIP(hipStreamSynchronize(ss));
        unsigned long long tot = 0;
        fprintf(stderr, "[mnf scatter] quad atomics per level:");
        for (int l = 0; l < 16; ++l) { fprintf(stderr, " %llu", h[l]); tot += h[l]; }
        fprintf(stderr, "  total %llu (upper bound n = %lld samples)\n", tot, (long long)n);
    }
#endif
    return rc;
}

}  // namespace mnf
