// The semantic surface mesh of a trained field on the device (gfx950): the iso-surface of a scalar lattice by marching tetrahedra on the Kuhn
// split, the lattice points of a trained field that are worth a density query, and the colours and classes of the vertices.
//   mnf_surface_extract         <- what the `extract_mesh` of the reference's nerfacc benchmarks does with skimage / mcubes on the host
//   mnf_surface_extract_observed   the same kernels with kObserved: a NaN point is unobserved, and neither its edges nor its tetrahedra emit
//   mnf_surface_lattice_points  <- estimator.binaries (visualization/vis_voxel.py reads the same grid), refined
//   mnf_surface_vertex_attrs    <- the colours and semantic labels of simulator/build_point_cloud_from_mesh.py, from the field's own outputs
// include/mi355nerf.h ("surface mesh") has the definition; every output byte of this unit is fixed by it.  Built with -ffp-contract=off: a
// vertex is a chain of separately rounded float32 operations, as numpy evaluates it (tests/surface_ref.py).
//
// Extraction.  A workgroup of 256 threads owns 256 CONSECUTIVE lattice points in lin order, one per thread; a thread also owns the cell
// whose lowest corner its point is.  Both output orders, vertices by (lin(p), type) and triangles by (cell, tetrahedron, triangle), are
// lexicographic in (x, y, z), so the outputs of a workgroup are one contiguous run of each list and two scans over the workgroups'
// totals place them: no per-point 64-bit counter exists anywhere.
//   surface_count_kernel  reads the point's value and its 7 upper neighbours (the ends of the 7 edge types and, at once, the other 7
//                         corners of its cell), and writes one word per point: bits 0..6 "edge type t carries a vertex", bit 7 "inside",
//                         bits 8.. the number of vertices the workgroup's earlier points own (<= 255 * 7).  Vertex and triangle totals
//                         of the workgroup go to two int64 arrays.
//   mnf_exclusive_scan_i64 twice.
//   surface_emit_kernel   reads that word alone (the 8 corner signs of the cell follow from it), writes the vertices its point owns and
//                         the triangles of its cell.  The index of the vertex on edge (q, t) is scan[q >> 8] + (word[q] >> 8) +
//                         popcount(word[q] & ((1 << t) - 1)): two loads that hit L1 / L2 next to the thread's own.
// The values are not staged in LDS: neighbouring lanes hold neighbouring z, so each of the 8 loads of the count pass is one coalesced row
// segment, and the rows of y + 1 and x + 1 are read again by the workgroups that own them (L2 hits).  Traffic per lattice point: 4 B of
// values from HBM and 4 B of words written in the count pass, 4 B of words read in the emit pass; everything else is per vertex or per
// triangle.  With kObserved the count pass adds bit 19 "this point is NaN" and bits 20..26 "the other end of edge type t is NaN" to the
// word (the prefix takes 11 bits, 8..18), an edge with a NaN end carries no vertex, and the emit pass drops the tetrahedra that hold a
// NaN corner; every tetrahedron holds corners 0 and 7, so a cell whose own point is NaN emits nothing and the other corners' signs still
// follow from the word.  The case table (which edges make the triangles of a tetrahedron, already oriented) is built at compile time from the
// rule of the header and sits in constant memory.
#include "reduce_dev.h"
#include "workspace.h"

namespace mnf {
namespace {

constexpr int kThreads = 256;                        // = 1 << kBlockShift, and what blocks_for counts in
constexpr int kBlockShift = 8;
constexpr int kMaxCells = 1024;                      // per axis: 1025^3 lattice points < 2^31

struct Lattice { int NX, NY, NZ, sx, sy; int n; float inv_sx, inv_sy; };   // points per axis; strides of x and y (z has 1); points in all; 1 / stride

inline bool make_lattice(int32_t X, int32_t Y, int32_t Z, Lattice *l) {
    if (X < 1 || Y < 1 || Z < 1 || X > kMaxCells || Y > kMaxCells || Z > kMaxCells) return false;
    const int64_t n = (int64_t)(X + 1) * (Y + 1) * (Z + 1);
    const int sx = (Y + 1) * (Z + 1), sy = Z + 1;
    *l = {X + 1, Y + 1, Z + 1, sx, sy, (int)n, 1.0f / (float)sx, 1.0f / (float)sy};
    return true;
}

// ---------------------------------------------------------------------------------------------------------------- the case table
// A cube corner is the 3-bit number dx | dy << 1 | dz << 2.  Edge type t runs along the corner kTypeCorner[t]: (1,0,0), (0,1,0), (0,0,1),
// (1,1,0), (1,0,1), (0,1,1), (1,1,1).
constexpr int kTypeCorner[7] = {1, 2, 4, 3, 5, 6, 7};
constexpr int kCornerType[8] = {-1, 0, 1, 3, 2, 4, 5, 6};
constexpr int kPerm[6][2] = {{0, 1}, {0, 2}, {1, 0}, {1, 2}, {2, 0}, {2, 1}};        // the first two axes of the k-th permutation

// entry [k][s], s = the inside bits of tetrahedron k's vertices 0..3: bits 0..1 the number of triangles, then 18 bits per triangle:
// three crossings of 6 bits each = owner corner | edge type << 3
struct CaseTable { uint64_t e[6][16]; };

constexpr CaseTable make_case_table() {
    CaseTable T{};
    for (int k = 0; k < 6; ++k) {
        const int corner[4] = {0, 1 << kPerm[k][0], (1 << kPerm[k][0]) | (1 << kPerm[k][1]), 7};
        for (int s = 1; s < 15; ++s) {
            int in[4] = {0, 0, 0, 0}, out[4] = {0, 0, 0, 0}, ni = 0, no = 0;
            for (int v = 0; v < 4; ++v) {
                if ((s >> v) & 1) in[ni++] = v; else out[no++] = v;
            }
            int tri[2][3][2] = {};                   // [triangle][crossing] = {tetrahedron vertex, tetrahedron vertex}
            int nt = 1;
            if (ni == 1) {
                for (int j = 0; j < 3; ++j) { tri[0][j][0] = in[0]; tri[0][j][1] = out[j]; }
            } else if (ni == 3) {
                for (int j = 0; j < 3; ++j) { tri[0][j][0] = in[j]; tri[0][j][1] = out[0]; }
            } else {
                nt = 2;
                const int a = in[0], b = in[1], c = out[0], d = out[1];
                tri[0][0][0] = a; tri[0][0][1] = c; tri[0][1][0] = a; tri[0][1][1] = d; tri[0][2][0] = b; tri[0][2][1] = d;
                tri[1][0][0] = a; tri[1][0][1] = c; tri[1][1][0] = b; tri[1][1][1] = d; tri[1][2][0] = b; tri[1][2][1] = c;
            }
            // w = mean(outside) - mean(inside), times ni * no; crossings at the midpoints, times 2: all integers
            int w[3] = {0, 0, 0};
            for (int ax = 0; ax < 3; ++ax) {
                int so = 0, si = 0;
                for (int j = 0; j < no; ++j) so += (corner[out[j]] >> ax) & 1;
                for (int j = 0; j < ni; ++j) si += (corner[in[j]] >> ax) & 1;
                w[ax] = so * ni - si * no;
            }
            uint64_t entry = (uint64_t)nt;
            for (int t = 0; t < nt; ++t) {
                int q[3][3] = {};
                for (int j = 0; j < 3; ++j)
                    for (int ax = 0; ax < 3; ++ax) q[j][ax] = ((corner[tri[t][j][0]] >> ax) & 1) + ((corner[tri[t][j][1]] >> ax) & 1);
                const int u[3] = {q[1][0] - q[0][0], q[1][1] - q[0][1], q[1][2] - q[0][2]};
                const int v[3] = {q[2][0] - q[0][0], q[2][1] - q[0][1], q[2][2] - q[0][2]};
                const int dot = (u[1] * v[2] - u[2] * v[1]) * w[0] + (u[2] * v[0] - u[0] * v[2]) * w[1] + (u[0] * v[1] - u[1] * v[0]) * w[2];
                const int order[3] = {0, dot < 0 ? 2 : 1, dot < 0 ? 1 : 2};
                uint64_t packed = 0;
                for (int j = 0; j < 3; ++j) {
                    const int a = tri[t][order[j]][0], b = tri[t][order[j]][1];
                    const int lo = a < b ? a : b, hi = a < b ? b : a;
                    const int code = corner[lo] | (kCornerType[corner[hi] ^ corner[lo]] << 3);
                    packed |= (uint64_t)code << (6 * j);
                }
                entry |= packed << (2 + 18 * t);
            }
            T.e[k][s] = entry;
        }
    }
    return T;
}

__constant__ CaseTable kCases = make_case_table();

// ---------------------------------------------------------------------------------------------------------------- shared pieces
// exclusive prefix over the workgroup of a small count per thread; *all = the workgroup's total.  One use per kernel.
__device__ __forceinline__ unsigned block_exclusive(unsigned v, unsigned *all) {
    __shared__ unsigned wave_total[kThreads / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned inc = v;
    if (__ballot(v != 0u)) {                             // (uniform) most waves of a lattice hold nothing
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned u = __shfl_up(inc, d, 64);
            if (lane >= d) inc += u;
        }
    }
    if (lane == 63) wave_total[wave] = inc;
    __syncthreads();
    unsigned before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < kThreads / 64; ++w) {
        const unsigned n = wave_total[w];
        before += w < wave ? n : 0;
        total += n;
    }
    *all = total;
    return before + inc - v;
}

// a / d for 0 <= a < 2^31 whose quotient is at most 1025: the float estimate is off by less than one (three roundings of 2^-24 each on a
// quotient < 2^11), so one step either way makes it exact.  An integer division is some 30 instructions, and every lattice point pays two.
__device__ __forceinline__ int small_quotient(int a, int d, float inv_d, int &rem) {
    int q = (int)((float)a * inv_d);
    int r = a - q * d;
    if (r < 0) { --q; r += d; }
    else if (r >= d) { ++q; r -= d; }
    rem = r;
    return q;
}

__device__ __forceinline__ void point_of(const Lattice &L, int lin, int &x, int &y, int &z) {
    int r;
    x = small_quotient(lin, L.sx, L.inv_sx, r);
    y = small_quotient(r, L.sy, L.inv_sy, z);
}

// the inside bits of the 8 corners of the cell at a point, from the point's word (bit 7: inside; bits 0..6: the other end differs)
__device__ __forceinline__ unsigned cube_bits(unsigned word) {
    const unsigned in = (word >> 7) & 1u;
    unsigned cb = in;
#pragma unroll
    for (int c = 1; c < 8; ++c) cb |= (in ^ ((word >> kCornerType[c]) & 1u)) << c;
    return cb;
}

__device__ __forceinline__ unsigned tet_case(unsigned cb, int k) {
    const int c1 = 1 << kPerm[k][0], c2 = c1 | (1 << kPerm[k][1]);
    return (cb & 1u) | (((cb >> c1) & 1u) << 1) | (((cb >> c2) & 1u) << 2) | (((cb >> 7) & 1u) << 3);
}

__device__ __forceinline__ unsigned triangles_of(unsigned cb) {
    if (cb == 0u || cb == 0xffu) return 0;
    unsigned n = 0;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const int c = __popc(tet_case(cb, k));
        n += (c == 0 || c == 4) ? 0u : c == 2 ? 2u : 1u;
    }
    return n;
}

// kObserved: the NaN bits of the 8 corners of the cell at a point, from the point's word (bit 19: this point; bits 20..26: the other ends)
constexpr int kPrefixBits = 11;                      // a workgroup's earlier points own at most 255 * 7 vertices
constexpr unsigned kPrefixMask = (1u << kPrefixBits) - 1u;
constexpr int kNanShift = 8 + kPrefixBits;

__device__ __forceinline__ unsigned cube_nan_bits(unsigned word) {
    unsigned nb = (word >> kNanShift) & 1u;
#pragma unroll
    for (int c = 1; c < 8; ++c) nb |= ((word >> (kNanShift + 1 + kCornerType[c])) & 1u) << c;
    return nb;
}

// a tetrahedron with a NaN corner emits nothing: its case becomes 0
__device__ __forceinline__ bool tet_observed(unsigned nb, int k) {
    const int c1 = 1 << kPerm[k][0], c2 = c1 | (1 << kPerm[k][1]);
    return ((nb & 1u) | ((nb >> c1) & 1u) | ((nb >> c2) & 1u) | ((nb >> 7) & 1u)) == 0u;
}

__device__ __forceinline__ unsigned triangles_of_observed(unsigned cb, unsigned nb) {
    if (nb & 0x81u) return 0;                          // corners 0 and 7 belong to all six
    unsigned n = 0;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        if (!tet_observed(nb, k)) continue;
        const int c = __popc(tet_case(cb, k));
        n += (c == 0 || c == 4) ? 0u : c == 2 ? 2u : 1u;
    }
    return n;
}

// ---------------------------------------------------------------------------------------------------------------- count
template <bool kObserved>
__global__ void __launch_bounds__(kThreads) surface_count_kernel(const float *__restrict__ values, Lattice L, float iso, unsigned *__restrict__ words,
                                                                 int64_t *__restrict__ vblock, int64_t *__restrict__ tblock) {
    const int64_t lin64 = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    unsigned bits = 0, nv = 0, nt = 0;
    if (lin64 < L.n) {
        const int lin = (int)lin64;
        int x, y, z;
        point_of(L, lin, x, y, z);
        const float a = values[lin];
        const bool in = a > iso, a_nan = kObserved && a != a;
        const bool hx = x + 1 < L.NX, hy = y + 1 < L.NY, hz = z + 1 < L.NZ;
        unsigned nans = a_nan ? 1u : 0u, diff = 0;                                    // diff: the ends differ, NaN or not (the corners' signs)
#pragma unroll
        for (int t = 0; t < 7; ++t) {
            const int c = kTypeCorner[t], dx = c & 1, dy = (c >> 1) & 1, dz = c >> 2;
            if ((dx && !hx) || (dy && !hy) || (dz && !hz)) continue;                  // the other end is not a lattice point: no such edge
            const float b = values[lin + dx * L.sx + dy * L.sy + dz];
            const bool other = b > iso;
            diff |= (other != in ? 1u : 0u) << t;
            if (kObserved) nans |= (b != b ? 1u : 0u) << (t + 1);
        }
        if (kObserved) {
            bits = a_nan ? 0u : diff & ~(nans >> 1);                                   // an edge with a NaN end carries no vertex
            nv = __popc(bits);
            // a NaN end is outside, as `diff` has it; where it was masked out of `bits` the emit pass reads the corner's sign as this point's,
            // which only tetrahedra with a NaN corner see
            if (!a_nan && hx && hy && hz) nt = triangles_of_observed(cube_bits(diff | ((in ? 1u : 0u) << 7)), cube_nan_bits(nans << kNanShift));
            bits |= ((in ? 1u : 0u) << 7) | (nans << kNanShift);
        } else {
            bits = diff;
            nv = __popc(bits);
            bits |= (in ? 1u : 0u) << 7;
            if (nv && hx && hy && hz) nt = triangles_of(cube_bits(bits));             // no edge of the point is cut: its cell has one sign
        }
    }
    unsigned all;
    const unsigned before = block_exclusive(nv | (nt << 16), &all);                    // <= 1792 and <= 3072 per workgroup: no carry between the halves
    if (lin64 < L.n) words[lin64] = ((before & kPrefixMask) << 8) | bits;
    if (threadIdx.x == 0) { vblock[blockIdx.x] = all & 0xffffu; tblock[blockIdx.x] = all >> 16; }
}

// ---------------------------------------------------------------------------------------------------------------- emit
__device__ __forceinline__ float lattice_difference(const float *__restrict__ v, int lin, int i, int n, int stride) {
    float d;
    if (i > 0 && i < n - 1) d = (v[lin + stride] - v[lin - stride]) * 0.5f;
    else if (i == 0) d = v[lin + stride] - v[lin];
    else d = v[lin] - v[lin - stride];
    return d - d == 0.0f ? d : 0.0f;
}

__device__ __forceinline__ int64_t vertex_index(const unsigned *__restrict__ words, const int64_t *__restrict__ vbase, int lin, int type) {
    const unsigned w = words[lin];
    return vbase[lin >> kBlockShift] + (int64_t)((w >> 8) & kPrefixMask) + __popc(w & ((1u << type) - 1u));
}

struct Frame { float o[3], s[3]; };

template <bool kObserved>
__global__ void __launch_bounds__(kThreads) surface_emit_kernel(const float *__restrict__ values, Lattice L, float iso, Frame F, const unsigned *__restrict__ words,
                                                                const int64_t *__restrict__ vbase, const int64_t *__restrict__ tbase,
                                                                const int64_t *__restrict__ totals, int64_t max_v, int64_t max_t,
                                                                float *__restrict__ positions, float *__restrict__ normals, int32_t *__restrict__ triangles,
                                                                int64_t *__restrict__ info) {
    const int64_t lin64 = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (lin64 == 0) {
        const int64_t V = totals[0], T = totals[1];
        info[0] = V; info[1] = T; info[2] = V > max_v ? V - max_v : 0; info[3] = T > max_t ? T - max_t : 0;
    }
    unsigned word = 0, nt = 0, cb = 0, nb = 0;
    int lin = 0, x = 0, y = 0, z = 0;
    if (lin64 < L.n) {
        lin = (int)lin64;
        word = words[lin];
        point_of(L, lin, x, y, z);
        if ((word & 0x7fu) && x + 1 < L.NX && y + 1 < L.NY && z + 1 < L.NZ) {
            cb = cube_bits(word);                                                     // kObserved: right for every corner of a tetrahedron that emits
            if (kObserved) { nb = cube_nan_bits(word); nt = triangles_of_observed(cb, nb); }
            else nt = triangles_of(cb);
        }
    }
    unsigned all;
    const unsigned tri_before = block_exclusive(nt, &all);
    // the vertices this point owns
    const unsigned mask = word & 0x7fu;
    if (mask) {
        const int64_t first = vbase[blockIdx.x] + (int64_t)((word >> 8) & kPrefixMask);
        const float a = values[lin];
        float ga[3];
        ga[0] = lattice_difference(values, lin, x, L.NX, L.sx);
        ga[1] = lattice_difference(values, lin, y, L.NY, L.sy);
        ga[2] = lattice_difference(values, lin, z, L.NZ, 1);
        int k = 0;
#pragma unroll
        for (int t = 0; t < 7; ++t) {
            if (!((mask >> t) & 1u)) continue;
            const int64_t r = first + k++;
            if (r >= max_v) break;                                                    // ranks ascend with t
            const int c = kTypeCorner[t], dx = c & 1, dy = (c >> 1) & 1, dz = c >> 2;
            const int other = lin + dx * L.sx + dy * L.sy + dz;
            const float b = values[other];
            float tt = 0.5f;
            if (a - a == 0.0f && b - b == 0.0f) tt = (iso - a) / (b - a);
            positions[3 * r + 0] = ((float)x + tt * (float)dx) * F.s[0] + F.o[0];
            positions[3 * r + 1] = ((float)y + tt * (float)dy) * F.s[1] + F.o[1];
            positions[3 * r + 2] = ((float)z + tt * (float)dz) * F.s[2] + F.o[2];
            float gb[3];
            gb[0] = lattice_difference(values, other, x + dx, L.NX, L.sx);
            gb[1] = lattice_difference(values, other, y + dy, L.NY, L.sy);
            gb[2] = lattice_difference(values, other, z + dz, L.NZ, 1);
            float m[3];
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) {
                const float g = ga[ax] + tt * (gb[ax] - ga[ax]);
                m[ax] = (-g) / F.s[ax];
            }
            const float len = sqrtf((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2]);
            const bool ok = len > 0.0f && len - len == 0.0f;
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) normals[3 * r + ax] = ok ? m[ax] / len : 0.0f;
        }
    }
    // the triangles of this point's cell
    if (nt) {
        int64_t r = tbase[blockIdx.x] + (int64_t)tri_before;
#pragma unroll 1
        for (int k = 0; k < 6; ++k) {
            if (kObserved && !tet_observed(nb, k)) continue;
            uint64_t e = kCases.e[k][tet_case(cb, k)];
            const int n = (int)(e & 3u);
            e >>= 2;
            for (int j = 0; j < n; ++j, ++r, e >>= 18) {
                if (r >= max_t) return;                                               // ranks ascend
                int64_t idx[3];
#pragma unroll
                for (int q = 0; q < 3; ++q) {
                    const int code = (int)(e >> (6 * q)) & 63, c = code & 7;
                    idx[q] = vertex_index(words, vbase, lin + (c & 1) * L.sx + ((c >> 1) & 1) * L.sy + (c >> 2), code >> 3);
                }
                if (idx[0] >= max_v || idx[1] >= max_v || idx[2] >= max_v) continue;  // counted, not written
                triangles[3 * r + 0] = (int32_t)idx[0]; triangles[3 * r + 1] = (int32_t)idx[1]; triangles[3 * r + 2] = (int32_t)idx[2];
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- measure
__global__ void __launch_bounds__(kThreads) surface_measure_kernel(const float *__restrict__ positions, const int32_t *__restrict__ triangles,
                                                                   const int64_t *__restrict__ info, int64_t max_v, int64_t max_t, double *__restrict__ out) {
    __shared__ double red[kThreads / 64][2];
    const int64_t nv = info[0] < max_v ? info[0] : max_v, ntri = info[1] < max_t ? info[1] : max_t;
    double area = 0.0, vol = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < ntri; i += (int64_t)gridDim.x * kThreads) {
        const int64_t ia = triangles[3 * i], ib = triangles[3 * i + 1], ic = triangles[3 * i + 2];
        if (ia < 0 || ia >= nv || ib < 0 || ib >= nv || ic < 0 || ic >= nv) continue;  // not a triangle of this mesh: nothing is read for it
        double a[3], b[3], c[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) { a[k] = (double)positions[3 * ia + k]; b[k] = (double)positions[3 * ib + k]; c[k] = (double)positions[3 * ic + k]; }
        const double u0 = b[0] - a[0], u1 = b[1] - a[1], u2 = b[2] - a[2], v0 = c[0] - a[0], v1 = c[1] - a[1], v2 = c[2] - a[2];
        const double n0 = u1 * v2 - u2 * v1, n1 = u2 * v0 - u0 * v2, n2 = u0 * v1 - u1 * v0;
        area += 0.5 * sqrt((n0 * n0 + n1 * n1) + n2 * n2);
        const double c0 = b[1] * c[2] - b[2] * c[1], c1 = b[2] * c[0] - b[0] * c[2], c2 = b[0] * c[1] - b[1] * c[0];
        vol += ((a[0] * c0 + a[1] * c1) + a[2] * c2) / 6.0;
    }
    wave_sum_each(area, vol);
    if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6][0] = area; red[threadIdx.x >> 6][1] = vol; }
    __syncthreads();
    if (threadIdx.x < 2) {
        const int k = threadIdx.x;
        atomicAdd(out + k, (red[0][k] + red[1][k]) + (red[2][k] + red[3][k]));
    }
}

// ---------------------------------------------------------------------------------------------------------------- lattice points
struct Refined { int R[3]; int shift; Lattice L; };

inline bool make_refined(int32_t RX, int32_t RY, int32_t RZ, int32_t refine, Refined *r) {
    if (RX < 1 || RY < 1 || RZ < 1 || RX > kMaxCells || RY > kMaxCells || RZ > kMaxCells) return false;
    if (refine != 1 && refine != 2 && refine != 4 && refine != 8) return false;
    r->R[0] = RX; r->R[1] = RY; r->R[2] = RZ;
    r->shift = refine == 1 ? 0 : refine == 2 ? 1 : refine == 4 ? 2 : 3;
    return make_lattice(RX * refine, RY * refine, RZ * refine, &r->L);
}

// near[c] = 1 where a cell of the 3 x 3 x 3 neighbourhood of c, clipped at the grid, is occupied
__global__ void __launch_bounds__(kThreads) surface_dilate_kernel(const uint8_t *__restrict__ binaries, int RX, int RY, int RZ, uint8_t *__restrict__ near) {
    const int64_t c = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (c >= (int64_t)RX * RY * RZ) return;
    const int x = (int)(c / ((int64_t)RY * RZ)), r = (int)(c - (int64_t)x * RY * RZ), y = r / RZ, z = r - y * RZ;
    bool any = false;
    for (int i = x > 0 ? x - 1 : 0; i <= (x + 1 < RX ? x + 1 : RX - 1); ++i)
        for (int j = y > 0 ? y - 1 : 0; j <= (y + 1 < RY ? y + 1 : RY - 1); ++j)
            for (int k = z > 0 ? z - 1 : 0; k <= (z + 1 < RZ ? z + 1 : RZ - 1); ++k) any = any || binaries[((int64_t)i * RY + j) * RZ + k] != 0;
    near[c] = any ? 1 : 0;
}

// a lattice point touches the cells (i - 1) >> shift and i >> shift of each axis, clipped at the grid: one cell, or two where i is a multiple of refine
__device__ __forceinline__ bool point_listed(const uint8_t *__restrict__ near, const Refined &G, int x, int y, int z) {
    const int p[3] = {x, y, z};
    int lo[3], hi[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        lo[k] = p[k] > 0 ? (p[k] - 1) >> G.shift : 0;
        hi[k] = (p[k] >> G.shift) < G.R[k] ? p[k] >> G.shift : G.R[k] - 1;
    }
    bool any = false;
    for (int i = lo[0]; i <= hi[0]; ++i)
        for (int j = lo[1]; j <= hi[1]; ++j)
            for (int k = lo[2]; k <= hi[2]; ++k) any = any || near[((int64_t)i * G.R[1] + j) * G.R[2] + k] != 0;
    return any;
}

__global__ void __launch_bounds__(kThreads) surface_points_count_kernel(const uint8_t *__restrict__ near, Refined G, int64_t *__restrict__ pblock) {
    const int64_t lin = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    unsigned listed = 0;
    if (lin < G.L.n) {
        int x, y, z;
        point_of(G.L, (int)lin, x, y, z);
        listed = point_listed(near, G, x, y, z) ? 1u : 0u;
    }
    unsigned all;
    block_exclusive(listed, &all);
    if (threadIdx.x == 0) pblock[blockIdx.x] = all;
}

__global__ void __launch_bounds__(kThreads) surface_points_emit_kernel(const uint8_t *__restrict__ near, Refined G, Frame F, const int64_t *__restrict__ pbase,
                                                                       const int64_t *__restrict__ total, int64_t max_points, int32_t *__restrict__ lins,
                                                                       float *__restrict__ positions, int64_t *__restrict__ info) {
    const int64_t lin = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (lin == 0) { info[0] = total[0]; info[1] = total[0] > max_points ? total[0] - max_points : 0; }
    unsigned listed = 0;
    int x = 0, y = 0, z = 0;
    if (lin < G.L.n) {
        point_of(G.L, (int)lin, x, y, z);
        listed = point_listed(near, G, x, y, z) ? 1u : 0u;
    }
    unsigned all;
    const unsigned before = block_exclusive(listed, &all);
    if (!listed) return;
    const int64_t r = pbase[blockIdx.x] + (int64_t)before;
    if (r >= max_points) return;
    lins[r] = (int32_t)lin;
    positions[3 * r + 0] = F.o[0] + (float)x * F.s[0];
    positions[3 * r + 1] = F.o[1] + (float)y * F.s[1];
    positions[3 * r + 2] = F.o[2] + (float)z * F.s[2];
}

__global__ void __launch_bounds__(kThreads) surface_scatter_kernel(const float *__restrict__ density, const int32_t *__restrict__ lins, const int64_t *__restrict__ info,
                                                                   int64_t max_points, float *__restrict__ values, int64_t n_values) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const int64_t n = info[0] < max_points ? info[0] : max_points;
    if (i >= n) return;
    const int64_t lin = lins[i];
    if (lin >= 0 && lin < n_values) values[lin] = density[i];
}

// ---------------------------------------------------------------------------------------------------------------- vertex attributes
__device__ __forceinline__ uint8_t colour_byte(float c) {
    if (c != c) return 0;
    const float u = fminf(fmaxf(c, 0.0f), 1.0f);
    return (uint8_t)(u * 255.0f + 0.5f);
}

__global__ void __launch_bounds__(kThreads) surface_attrs_kernel(const float *__restrict__ rgb, const float *__restrict__ sem, int64_t n, int C,
                                                                 const uint8_t *__restrict__ palette, uint8_t *__restrict__ colour, int32_t *__restrict__ label,
                                                                 uint8_t *__restrict__ sem_colour) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    if (colour) {
#pragma unroll
        for (int k = 0; k < 3; ++k) colour[3 * i + k] = colour_byte(rgb[3 * i + k]);
    }
    if (!label && !sem_colour) return;
    int best = -1;
    float top = 0.0f;
    bool nan = false;
    for (int c = 0; c < C; ++c) {
        const float v = sem[i * C + c];
        nan = nan || v != v;
        if (best < 0 || v > top) { best = c; top = v; }
    }
    if (nan) best = -1;
    if (label) label[i] = best;
    if (sem_colour) {
#pragma unroll
        for (int k = 0; k < 3; ++k) sem_colour[3 * i + k] = best >= 0 ? palette[3 * best + k] : (uint8_t)0;
    }
}

// ---------------------------------------------------------------------------------------------------------------- workspaces
struct ExtractWs { unsigned *words; int64_t *vblock, *tblock, *vbase, *tbase, *totals, *scan; int64_t bytes; };

inline ExtractWs carve_extract(void *base, int64_t n, int64_t nb) {
    Carver c(base, 8);
    ExtractWs w;
    w.words = c.take<unsigned>(n);
    w.vblock = c.take<int64_t>(nb);
    w.tblock = c.take<int64_t>(nb);
    w.vbase = c.take<int64_t>(nb);
    w.tbase = c.take<int64_t>(nb);
    w.totals = c.take<int64_t>(2);
    w.scan = (int64_t *)c.take(scan_bytes(nb));
    w.bytes = c.bytes();
    return w;
}

struct PointsWs { uint8_t *near; int64_t *pblock, *pbase, *total, *scan; int64_t bytes; };

inline PointsWs carve_points(void *base, int64_t cells, int64_t nb) {
    Carver c(base, 8);
    PointsWs w;
    w.near = c.take<uint8_t>(cells);
    w.pblock = c.take<int64_t>(nb);
    w.pbase = c.take<int64_t>(nb);
    w.total = c.take<int64_t>(1);
    w.scan = (int64_t *)c.take(scan_bytes(nb));
    w.bytes = c.bytes();
    return w;
}

inline bool finite_f(float v) { return v - v == 0.0f; }

}  // namespace
}  // namespace mnf

using namespace mnf;

extern "C" int64_t mnf_surface_extract_workspace_bytes(int32_t cells_x, int32_t cells_y, int32_t cells_z) {
    Lattice L;
    if (!make_lattice(cells_x, cells_y, cells_z, &L)) return 0;
    return carve_extract(nullptr, L.n, blocks_for(L.n)).bytes;
}

// both entries: `observed` picks the kernels' rule for NaN
static int surface_extract(bool observed, const float *values, int32_t cells_x, int32_t cells_y, int32_t cells_z, float iso, const float *origin_host,
                           const float *step_host, int64_t max_vertices, int64_t max_triangles, float *positions, float *normals, int32_t *triangles,
                           int64_t *info, void *workspace, int64_t workspace_bytes, mnf_stream_t stream) {
    Lattice L;
    MNF_REQUIRE(make_lattice(cells_x, cells_y, cells_z, &L), "surface_extract: cells per axis must lie in 1 .. %d (got %d x %d x %d)", kMaxCells, cells_x,
                cells_y, cells_z);
    MNF_REQUIRE(finite_f(iso), "surface_extract: iso is not finite");
    MNF_REQUIRE(origin_host, "surface_extract: origin is null");
    MNF_REQUIRE(step_host, "surface_extract: step is null");
    for (int k = 0; k < 3; ++k)
        MNF_REQUIRE(step_host[k] > 0.0f && finite_f(step_host[k]), "surface_extract: step must be positive and finite (got %g on axis %d)", (double)step_host[k], k);
    MNF_REQUIRE(max_vertices >= 0 && max_vertices <= 0x7fffffff, "surface_extract: max_vertices outside [0, 2^31) (got %lld)", (long long)max_vertices);
    MNF_REQUIRE(max_triangles >= 0 && max_triangles <= 0x7fffffff, "surface_extract: max_triangles outside [0, 2^31) (got %lld)", (long long)max_triangles);
    MNF_REQUIRE(values, "surface_extract: values is null");
    MNF_REQUIRE(positions || max_vertices == 0, "surface_extract: positions is null");
    MNF_REQUIRE(normals || max_vertices == 0, "surface_extract: normals is null");
    MNF_REQUIRE(triangles || max_triangles == 0, "surface_extract: triangles is null");
    MNF_REQUIRE(info, "surface_extract: info is null");
    MNF_REQUIRE(aligned8(info), "surface_extract: info must be 8-byte aligned");
    MNF_REQUIRE(workspace, "surface_extract: workspace is null");
    MNF_REQUIRE(aligned8(workspace), "surface_extract: workspace must be 8-byte aligned");
    const int64_t nb = blocks_for(L.n);
    const ExtractWs w = carve_extract(workspace, L.n, nb);
    MNF_REQUIRE(workspace_bytes >= w.bytes, "surface_extract: workspace too small (%lld < %lld bytes)", (long long)workspace_bytes, (long long)w.bytes);
    Frame F;
    for (int k = 0; k < 3; ++k) { F.o[k] = origin_host[k]; F.s[k] = step_host[k]; }
    hipStream_t s = as_stream(stream);
    ProfScope prof(observed ? "surface_extract_observed" : "surface_extract", s);
    if (observed) hipLaunchKernelGGL(surface_count_kernel<true>, dim3((unsigned)nb), dim3(kThreads), 0, s, values, L, iso, w.words, w.vblock, w.tblock);
    else hipLaunchKernelGGL(surface_count_kernel<false>, dim3((unsigned)nb), dim3(kThreads), 0, s, values, L, iso, w.words, w.vblock, w.tblock);
    int rc = launch_status("surface_count_kernel");
    if (rc) return rc;
    rc = mnf_exclusive_scan_i64(w.vblock, nb, w.vbase, w.totals, w.scan, scan_bytes(nb), stream);
    if (rc) return rc;
    rc = mnf_exclusive_scan_i64(w.tblock, nb, w.tbase, w.totals + 1, w.scan, scan_bytes(nb), stream);
    if (rc) return rc;
    if (observed)
        hipLaunchKernelGGL(surface_emit_kernel<true>, dim3((unsigned)nb), dim3(kThreads), 0, s, values, L, iso, F, w.words, w.vbase, w.tbase, w.totals,
                           max_vertices, max_triangles, positions, normals, triangles, info);
    else
        hipLaunchKernelGGL(surface_emit_kernel<false>, dim3((unsigned)nb), dim3(kThreads), 0, s, values, L, iso, F, w.words, w.vbase, w.tbase, w.totals,
                           max_vertices, max_triangles, positions, normals, triangles, info);
    return launch_status("surface_emit_kernel");
}

extern "C" int mnf_surface_extract(const float *values, int32_t cells_x, int32_t cells_y, int32_t cells_z, float iso, const float *origin_host,
                                   const float *step_host, int64_t max_vertices, int64_t max_triangles, float *positions, float *normals,
                                   int32_t *triangles, int64_t *info, void *workspace, int64_t workspace_bytes, mnf_stream_t stream) {
    return surface_extract(false, values, cells_x, cells_y, cells_z, iso, origin_host, step_host, max_vertices, max_triangles, positions, normals, triangles,
                           info, workspace, workspace_bytes, stream);
}

extern "C" int mnf_surface_extract_observed(const float *values, int32_t cells_x, int32_t cells_y, int32_t cells_z, float iso, const float *origin_host,
                                            const float *step_host, int64_t max_vertices, int64_t max_triangles, float *positions, float *normals,
                                            int32_t *triangles, int64_t *info, void *workspace, int64_t workspace_bytes, mnf_stream_t stream) {
    return surface_extract(true, values, cells_x, cells_y, cells_z, iso, origin_host, step_host, max_vertices, max_triangles, positions, normals, triangles,
                           info, workspace, workspace_bytes, stream);
}

extern "C" int mnf_surface_measure(const float *positions, const int32_t *triangles, const int64_t *info, int64_t max_vertices, int64_t max_triangles,
                                   double *out, mnf_stream_t stream) {
    MNF_REQUIRE(max_vertices >= 0 && max_vertices <= 0x7fffffff, "surface_measure: max_vertices outside [0, 2^31) (got %lld)", (long long)max_vertices);
    MNF_REQUIRE(max_triangles >= 0 && max_triangles <= 0x7fffffff, "surface_measure: max_triangles outside [0, 2^31) (got %lld)", (long long)max_triangles);
    MNF_REQUIRE(positions || max_vertices == 0, "surface_measure: positions is null");
    MNF_REQUIRE(triangles || max_triangles == 0, "surface_measure: triangles is null");
    MNF_REQUIRE(info, "surface_measure: info is null");
    MNF_REQUIRE(out, "surface_measure: out is null");
    MNF_REQUIRE(aligned8(info) && aligned8(out), "surface_measure: info and out must be 8-byte aligned");
    hipStream_t s = as_stream(stream);
    ProfScope prof("surface_measure", s);
    MNF_HIP(hipMemsetAsync(out, 0, 2 * sizeof(double), s));
    if (max_triangles == 0 || max_vertices == 0) return MNF_OK;
    const unsigned nb = blocks_for(max_triangles) < 2048u ? blocks_for(max_triangles) : 2048u;
    hipLaunchKernelGGL(surface_measure_kernel, dim3(nb), dim3(kThreads), 0, s, positions, triangles, info, max_vertices, max_triangles, out);
    return launch_status("surface_measure_kernel");
}

extern "C" int64_t mnf_surface_lattice_points_workspace_bytes(int32_t res_x, int32_t res_y, int32_t res_z, int32_t refine) {
    Refined G;
    if (!make_refined(res_x, res_y, res_z, refine, &G)) return 0;
    return carve_points(nullptr, (int64_t)res_x * res_y * res_z, blocks_for(G.L.n)).bytes;
}

extern "C" int mnf_surface_lattice_points(const uint8_t *binaries, int32_t res_x, int32_t res_y, int32_t res_z, int32_t refine, const float *aabb_host,
                                          int64_t max_points, int32_t *lin, float *positions, int64_t *info, void *workspace, int64_t workspace_bytes,
                                          mnf_stream_t stream) {
    Refined G;
    MNF_REQUIRE(refine == 1 || refine == 2 || refine == 4 || refine == 8, "surface_lattice_points: refine is 1, 2, 4 or 8 (got %d)", refine);
    MNF_REQUIRE(make_refined(res_x, res_y, res_z, refine, &G), "surface_lattice_points: resolution x refine must lie in 1 .. %d per axis (got %d x %d x %d x %d)",
                kMaxCells, res_x, res_y, res_z, refine);
    MNF_REQUIRE(aabb_host, "surface_lattice_points: aabb is null");
    Frame F;
    for (int k = 0; k < 3; ++k) {
        F.o[k] = aabb_host[k];
        F.s[k] = (aabb_host[3 + k] - aabb_host[k]) / (float)(G.R[k] * refine);
        MNF_REQUIRE(F.s[k] > 0.0f && finite_f(F.s[k]) && finite_f(F.o[k]), "surface_lattice_points: the aabb must be finite and not empty (axis %d)", k);
    }
    MNF_REQUIRE(max_points >= 0 && max_points <= 0x7fffffff, "surface_lattice_points: max_points outside [0, 2^31) (got %lld)", (long long)max_points);
    MNF_REQUIRE(binaries, "surface_lattice_points: binaries is null");
    MNF_REQUIRE(lin || max_points == 0, "surface_lattice_points: lin is null");
    MNF_REQUIRE(positions || max_points == 0, "surface_lattice_points: positions is null");
    MNF_REQUIRE(info, "surface_lattice_points: info is null");
    MNF_REQUIRE(aligned8(info), "surface_lattice_points: info must be 8-byte aligned");
    MNF_REQUIRE(workspace, "surface_lattice_points: workspace is null");
    MNF_REQUIRE(aligned8(workspace), "surface_lattice_points: workspace must be 8-byte aligned");
    const int64_t cells = (int64_t)res_x * res_y * res_z, nb = blocks_for(G.L.n);
    const PointsWs w = carve_points(workspace, cells, nb);
    MNF_REQUIRE(workspace_bytes >= w.bytes, "surface_lattice_points: workspace too small (%lld < %lld bytes)", (long long)workspace_bytes, (long long)w.bytes);
    hipStream_t s = as_stream(stream);
    ProfScope prof("surface_lattice_points", s);
    hipLaunchKernelGGL(surface_dilate_kernel, dim3(blocks_for(cells)), dim3(kThreads), 0, s, binaries, res_x, res_y, res_z, w.near);
    int rc = launch_status("surface_dilate_kernel");
    if (rc) return rc;
    hipLaunchKernelGGL(surface_points_count_kernel, dim3((unsigned)nb), dim3(kThreads), 0, s, w.near, G, w.pblock);
    rc = launch_status("surface_points_count_kernel");
    if (rc) return rc;
    rc = mnf_exclusive_scan_i64(w.pblock, nb, w.pbase, w.total, w.scan, scan_bytes(nb), stream);
    if (rc) return rc;
    hipLaunchKernelGGL(surface_points_emit_kernel, dim3((unsigned)nb), dim3(kThreads), 0, s, w.near, G, F, w.pbase, w.total, max_points, lin, positions, info);
    return launch_status("surface_points_emit_kernel");
}

extern "C" int mnf_surface_lattice_scatter(const float *density, const int32_t *lin, const int64_t *point_info, int64_t max_points, float *values,
                                           int64_t n_values, mnf_stream_t stream) {
    MNF_REQUIRE(max_points >= 0 && max_points <= 0x7fffffff, "surface_lattice_scatter: max_points outside [0, 2^31) (got %lld)", (long long)max_points);
    MNF_REQUIRE(n_values > 0 && n_values <= 0x7fffffff, "surface_lattice_scatter: n_values outside [1, 2^31) (got %lld)", (long long)n_values);
    MNF_REQUIRE(density || max_points == 0, "surface_lattice_scatter: density is null");
    MNF_REQUIRE(lin || max_points == 0, "surface_lattice_scatter: lin is null");
    MNF_REQUIRE(point_info, "surface_lattice_scatter: point_info is null");
    MNF_REQUIRE(aligned8(point_info), "surface_lattice_scatter: point_info must be 8-byte aligned");
    MNF_REQUIRE(values, "surface_lattice_scatter: values is null");
    hipStream_t s = as_stream(stream);
    ProfScope prof("surface_lattice_scatter", s);
    MNF_HIP(hipMemsetAsync(values, 0, (size_t)n_values * sizeof(float), s));
    if (max_points == 0) return MNF_OK;
    hipLaunchKernelGGL(surface_scatter_kernel, dim3(blocks_for(max_points)), dim3(kThreads), 0, s, density, lin, point_info, max_points, values, n_values);
    return launch_status("surface_scatter_kernel");
}

extern "C" int mnf_surface_vertex_attrs(const float *rgb, const float *sem, int64_t n, int32_t n_classes, const uint8_t *palette, uint8_t *colour,
                                        int32_t *label, uint8_t *sem_colour, mnf_stream_t stream) {
    MNF_REQUIRE(n >= 0 && n <= 0x7fffffff, "surface_vertex_attrs: n outside [0, 2^31) (got %lld)", (long long)n);
    MNF_REQUIRE(n_classes >= 1, "surface_vertex_attrs: n_classes must be at least 1 (got %d)", n_classes);
    MNF_REQUIRE(rgb || !colour || n == 0, "surface_vertex_attrs: rgb is null");
    MNF_REQUIRE(sem || (!label && !sem_colour) || n == 0, "surface_vertex_attrs: sem is null");
    MNF_REQUIRE(palette || !sem_colour || n == 0, "surface_vertex_attrs: sem_colour asks for a palette");
    if (n == 0 || (!colour && !label && !sem_colour)) return MNF_OK;
    hipStream_t s = as_stream(stream);
    ProfScope prof("surface_vertex_attrs", s);
    hipLaunchKernelGGL(surface_attrs_kernel, dim3(blocks_for(n)), dim3(kThreads), 0, s, rgb, sem, n, n_classes, palette, colour, label, sem_colour);
    return launch_status("surface_attrs_kernel");
}
