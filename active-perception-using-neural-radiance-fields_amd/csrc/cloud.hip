// The quality of the map as geometry, on the device (gfx950): points sampled on the triangles of a mesh, the nearest neighbour of every point of
// one cloud in another within a radius, and the reduction of those distances to the counts, sums and confusion matrix the metrics are made of.
//   mnf_cloud_sample_triangles  <- the sampling loop of simulator/build_point_cloud_from_mesh.py (per face: three vertices, then rows along the
//                                  first edge, each filled along the second)
//   mnf_cloud_nearest           <- the k-d-tree query an evaluation makes on the host (cKDTree.query(k = 1, distance_upper_bound))
//   mnf_cloud_distance_stats    <- accuracy / completion / precision / recall / confusion from the distances
// include/mi355nerf.h ("mesh quality") has the definition; every output byte of the first two is fixed by it.  Built with -ffp-contract=off: a
// sampled point is a chain of separately rounded float64 operations and a squared distance one of float32 operations, as numpy evaluates them
// (tests/cloud_ref.py).
//
// Sampling.  A wall triangle of 5 m holds 10^5 points at 1 cm and a chair's triangle ten, so the work is distributed by ROW = (triangle, k): the
// points p1 + (k res) n1 + (l res) n2, l = 0 .. count - 1.  Row 0 of a triangle is its three vertices, row 1 + k the k-th row of the loop.
//   cloud_tri_rows_kernel    one lane per triangle: rows of the triangle (0: an index out of range; 1: degenerate; 1 + ceil(d1 / res))
//   mnf_exclusive_scan_i64   row base per triangle, rows in all (R)
//   cloud_row_points_kernel  one lane per row slot: the triangle of the row (a binary search in the row bases), its point count
//   mnf_exclusive_scan_i64   point base per row, points in all
//   cloud_fill_kernel        one lane per output point: the row of the point (a binary search in the point bases), the point
// The geometry of a triangle (two square roots, six divisions in float64) is recomputed per row and per point from 36 bytes that sit in L2: the
// same operations in the same order give the same double everywhere, so nothing but the two scans is stored.
//
// Nearest neighbour.  A uniform cell list over the caller's box whose edge h is a little more than r_max (see make_cells for the margin).
//   cloud_bin_kernel      one lane per target and per query: the cell of the point, one atomic count per point; a query that is not finite gets
//                         its answer here
//   mnf_exclusive_scan_i64 twice: the first slot of every cell, for the targets and for the queries
//   cloud_place_kernel    counting sort: targets go to their cell's run as float4 (x, y, z, original index), queries as (original index, cell)
//   cloud_nearest_kernel  a workgroup of 256 lanes owns 256 consecutive SORTED queries, one per lane, and walks the cells they lie in: for a cell
//                         it streams the targets of the 3 x 3 x 3 neighbourhood through LDS, kStage at a time; the three z-neighbours of a
//                         column are consecutive cells, so the neighbourhood is 9 contiguous runs of the sorted targets.  Every lane of the
//                         cell reads the same LDS address (a broadcast, no bank conflict) and keeps (d2, index) with the lowest index on a tie,
//                         so the order inside a run (which the atomics of the sort decide) cannot change a result.  Answers go back to the
//                         queries' original places.
// Every loop is bounded by counts read once from the scans; no lane waits for another workgroup.
#include "reduce_dev.h"
#include "workspace.h"

namespace mnf {
namespace {

constexpr int kThreads = 256;
constexpr int64_t kMaxCount = 0x7fffffff;            // triangles, vertices, rows, points, queries, targets: all < 2^31
constexpr int64_t kCountCap = (int64_t)1 << 31;      // what a single row count or point count of a row saturates at
constexpr int kMaxAxisCells = 128;                   // cells per axis of the cell list: at most 2^21 cells
constexpr int kStage = 1024;                         // targets staged in LDS at a time (16 KiB)
constexpr int kMaxClasses = 1024;

inline bool finite_f(float v) { return v - v == 0.0f; }

// ---------------------------------------------------------------------------------------------------------------- sampling
// ceil(x) as a count: 0 for x <= 0 (numpy's arange of a non-positive length is empty) and for NaN, saturating at kCountCap
__device__ __forceinline__ int64_t count_of(double x) {
    if (!(x > 0.0)) return 0;
    const double c = ceil(x);
    return c >= (double)kCountCap ? kCountCap : (int64_t)c;
}

struct TriGeom { double p1[3], n1[3], n2[3], d1, d2; float v[3][3]; bool plain; };   // plain: rows exist beyond the vertices

// false: an index outside [0, V), the triangle gives nothing
__device__ __forceinline__ bool load_triangle(const float *__restrict__ positions, int64_t V, const int32_t *__restrict__ triangles, int64_t t, TriGeom &g) {
    const int64_t ia = triangles[3 * t], ib = triangles[3 * t + 1], ic = triangles[3 * t + 2];
    if (ia < 0 || ia >= V || ib < 0 || ib >= V || ic < 0 || ic >= V) return false;
    bool finite = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        g.v[0][k] = positions[3 * ia + k]; g.v[1][k] = positions[3 * ib + k]; g.v[2][k] = positions[3 * ic + k];
        finite = finite && g.v[0][k] - g.v[0][k] == 0.0f && g.v[1][k] - g.v[1][k] == 0.0f && g.v[2][k] - g.v[2][k] == 0.0f;
    }
    double e1[3], e2[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        g.p1[k] = (double)g.v[0][k];
        e1[k] = (double)g.v[1][k] - g.p1[k];
        e2[k] = (double)g.v[2][k] - g.p1[k];
    }
    g.d1 = sqrt((e1[0] * e1[0] + e1[1] * e1[1]) + e1[2] * e1[2]);
    g.d2 = sqrt((e2[0] * e2[0] + e2[1] * e2[1]) + e2[2] * e2[2]);
    g.plain = finite && g.d1 > 0.0 && g.d2 > 0.0;
    if (g.plain) {
#pragma unroll
        for (int k = 0; k < 3; ++k) { g.n1[k] = e1[k] / g.d1; g.n2[k] = e2[k] / g.d2; }
    }
    return true;
}

__global__ void __launch_bounds__(kThreads) cloud_tri_rows_kernel(const float *__restrict__ positions, int64_t V, const int32_t *__restrict__ triangles, int64_t T,
                                                                  double res, int64_t *__restrict__ tri_rows) {
    const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (t >= T) return;
    TriGeom g;
    int64_t rows = 0;
    if (load_triangle(positions, V, triangles, t, g)) rows = 1 + (g.plain ? count_of(g.d1 / res) : 0);
    tri_rows[t] = rows;
}

// the last i in [0, n) with base[i] <= x; base ascends and base[0] = 0 <= x
__device__ __forceinline__ int64_t last_not_above(const int64_t *__restrict__ base, int64_t n, int64_t x) {
    int64_t lo = 0, hi = n;                            // base[lo] <= x < base[hi] (base[n] = infinity)
    while (hi - lo > 1) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (base[mid] <= x) lo = mid; else hi = mid;
    }
    return lo;
}

__global__ void __launch_bounds__(kThreads) cloud_row_points_kernel(const float *__restrict__ positions, int64_t V, const int32_t *__restrict__ triangles, int64_t T,
                                                                    double res, const int64_t *__restrict__ tri_base, const int64_t *__restrict__ row_total,
                                                                    int64_t max_rows, int32_t *__restrict__ row_tri, int64_t *__restrict__ row_points) {
    const int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (r >= max_rows) return;
    const int64_t R = row_total[0];
    if (r >= R) { row_points[r] = 0; return; }          // also every slot of a mesh with more rows than max_rows is harmless: the fill writes nothing then
    const int64_t t = last_not_above(tri_base, T, r);    // triangles without rows share their base with the next one that has some: the last wins
    TriGeom g;
    int64_t n = 0;
    if (load_triangle(positions, V, triangles, t, g)) {
        const int64_t kr = r - tri_base[t];
        if (kr == 0) n = 3;
        else if (g.plain) {
            const double i = (double)(kr - 1) * res;
            const double b = ((g.d1 - i) * g.d2) / g.d1;
            n = count_of(b / res);
        }
    }
    row_tri[r] = (int32_t)t;
    row_points[r] = n;
}

__global__ void __launch_bounds__(kThreads) cloud_fill_kernel(const float *__restrict__ positions, int64_t V, const int32_t *__restrict__ triangles, double res,
                                                              const int64_t *__restrict__ tri_base, const int64_t *__restrict__ row_total, int64_t max_rows,
                                                              const int32_t *__restrict__ row_tri, const int64_t *__restrict__ row_base,
                                                              const int64_t *__restrict__ point_total, int64_t max_points, float *__restrict__ points,
                                                              int32_t *__restrict__ face, int64_t *__restrict__ info) {
    const int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const int64_t R = row_total[0], P = max_rows > 0 ? point_total[0] : 0;
    const bool refused = R > max_rows;
    if (p == 0) {
        info[0] = refused ? -1 : P;
        info[1] = refused ? R : (P > max_points ? P - max_points : 0);
    }
    if (refused || p >= P || p >= max_points) return;
    const int64_t r = last_not_above(row_base, R, p);    // rows without points share their base with the next one that has some
    const int64_t t = row_tri[r], kr = r - tri_base[t], l = p - row_base[r];
    TriGeom g;
    if (!load_triangle(positions, V, triangles, t, g)) return;                        // cannot be: such a triangle has no row
    float out[3];
    if (kr == 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) out[k] = l == 0 ? g.v[0][k] : l == 1 ? g.v[1][k] : g.v[2][k];
    } else {
        const double i = (double)(kr - 1) * res, j = (double)l * res;
#pragma unroll
        for (int k = 0; k < 3; ++k) out[k] = (float)((g.p1[k] + i * g.n1[k]) + j * g.n2[k]);
    }
    points[3 * p + 0] = out[0]; points[3 * p + 1] = out[1]; points[3 * p + 2] = out[2];
    face[p] = (int32_t)t;
}

struct SampleWs { int64_t *tri_rows, *tri_base, *row_points, *row_base, *totals, *scan; int32_t *row_tri; int64_t bytes; };

inline SampleWs carve_sample(void *base, int64_t T, int64_t max_rows) {
    Carver c(base, 8);
    SampleWs w;
    const int64_t longest = T > max_rows ? T : max_rows;
    w.tri_rows = c.take<int64_t>(T);
    w.tri_base = c.take<int64_t>(T);
    w.row_points = c.take<int64_t>(max_rows);
    w.row_base = c.take<int64_t>(max_rows);
    w.row_tri = c.take<int32_t>(max_rows);
    w.totals = c.take<int64_t>(2);
    w.scan = (int64_t *)c.take(scan_bytes(longest));
    w.bytes = c.bytes();
    return w;
}

inline bool sample_sizes_ok(int64_t T, int64_t max_rows) { return T >= 0 && T <= kMaxCount && max_rows >= 0 && max_rows <= kMaxCount; }

// ---------------------------------------------------------------------------------------------------------------- the cell list
// Cell of a coordinate p on an axis: min(max(floor(u), 0), c - 1) with u = ((double)p - lo) * inv_h, two float64 roundings.  The grid is DEFINED
// by inv_h (h = 1 / inv_h exactly), so the only errors of u are those two roundings: |u - u_true| <= 2 * 2^-53 * |u_true|; after the clamp only
// |u_true| <= 128 + 1 matters (beyond, both sides clamp to a border cell and the clamp is monotone), so the error is below 2^-44.
// A pair that mnf_cloud_nearest accepts has a float32 d2 <= fl(r_max r_max); dx, dx dx, the two sums and the product each round by 2^-24
// relative as long as nothing underflows; r_max >= 2^-60 (kMinRadius) keeps r_max r_max a normal float32 >= 2^-120, and a square of a difference
// that does underflow is off by at most 2^-150 absolute, 2^-30 of that.  So the true |q - t| on an axis is below r_max (1 + 2^-21).  make_cells takes h >= r_max (1 + 2^-10) up to one rounding of the quotient,
// hence |u_true(q) - u_true(t)| <= (1 + 2^-21) / (1 + 2^-10) (1 + 2^-52) < 1 - 2^-11, the computed u differ by less than 1 - 2^-11 + 2^-43 < 1,
// and floor() of two numbers less than 1 apart differs by at most 1; the monotone clamp keeps that.  So a target within r_max of a query is never
// two cells away, wherever the two lie: inside the box, outside it (they fall into border cells), or one of each.
struct Cells { double lo[3]; double inv_h; int c[3]; int n; };

constexpr float kMinRadius = 0x1p-60f;

inline bool radius_ok(float r_max) { return r_max >= kMinRadius && finite_f(r_max) && finite_f(r_max * r_max); }

inline bool make_cells(const float *box, float r_max, Cells *g) {
    if (!box || !radius_ok(r_max)) return false;
    double widest = 0.0;
    for (int k = 0; k < 3; ++k) {
        if (!finite_f(box[k]) || !finite_f(box[3 + k]) || box[3 + k] < box[k]) return false;
        const double e = (double)box[3 + k] - (double)box[k];
        widest = e > widest ? e : widest;
    }
    double h = (double)r_max * (1.0 + 1.0 / 1024.0);
    if (widest / kMaxAxisCells > h) h = widest / kMaxAxisCells;                          // a coarser list is as exact, only slower
    g->inv_h = 1.0 / h;
    if (!(g->inv_h > 0.0) || !finite_d(g->inv_h)) return false;
    g->n = 1;
    for (int k = 0; k < 3; ++k) {
        g->lo[k] = (double)box[k];
        const double u = ((double)box[3 + k] - g->lo[k]) * g->inv_h;
        const int c = (int)u + 1;                                                        // u <= 128 (1 + 2^-52)
        g->c[k] = c > kMaxAxisCells ? kMaxAxisCells : c;
        g->n *= g->c[k];
    }
    return true;
}

__device__ __forceinline__ int axis_cell(double p, double lo, double inv_h, int c) {
    const double u = (p - lo) * inv_h;
    return (int)fmin(fmax(floor(u), 0.0), (double)(c - 1));
}

// -1 for a point with a coordinate that is not finite
__device__ __forceinline__ int cell_of(const Cells &G, const float *__restrict__ p) {
    const float x = p[0], y = p[1], z = p[2];
    if (!(x - x == 0.0f && y - y == 0.0f && z - z == 0.0f)) return -1;
    const int cx = axis_cell((double)x, G.lo[0], G.inv_h, G.c[0]), cy = axis_cell((double)y, G.lo[1], G.inv_h, G.c[1]),
              cz = axis_cell((double)z, G.lo[2], G.inv_h, G.c[2]);
    return (cx * G.c[1] + cy) * G.c[2] + cz;
}

// lanes [0, m): targets; lanes [m, m + n): queries
__global__ void __launch_bounds__(kThreads) cloud_bin_kernel(const float *__restrict__ query, int64_t n, const float *__restrict__ target, int64_t m, Cells G,
                                                             float r_max, int32_t *__restrict__ tcell, int32_t *__restrict__ qcell, int64_t *__restrict__ tcount,
                                                             int64_t *__restrict__ qcount, int32_t *__restrict__ index, float *__restrict__ dist) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i < m) {
        const int c = cell_of(G, target + 3 * i);
        tcell[i] = c;
        if (c >= 0) atomicAdd((unsigned long long *)(tcount + c), 1ull);
    } else if (i < m + n) {
        const int64_t q = i - m;
        const int c = cell_of(G, query + 3 * q);
        qcell[q] = c;
        if (c >= 0) atomicAdd((unsigned long long *)(qcount + c), 1ull);
        else { index[q] = -1; dist[q] = r_max; }
    }
}

// the counts are used up as the runs fill: slot = start + (what is left of the count) - 1.  Which member gets which slot of its run is the atomics' affair.
__global__ void __launch_bounds__(kThreads) cloud_place_kernel(const float *__restrict__ target, int64_t n, int64_t m, const int32_t *__restrict__ tcell,
                                                               const int32_t *__restrict__ qcell, const int64_t *__restrict__ tstart, const int64_t *__restrict__ qstart,
                                                               int64_t *__restrict__ tcount, int64_t *__restrict__ qcount, float4 *__restrict__ tsorted,
                                                               int32_t *__restrict__ qsorted, int32_t *__restrict__ qsorted_cell) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i < m) {
        const int c = tcell[i];
        if (c < 0) return;
        const int64_t left = (int64_t)atomicAdd((unsigned long long *)(tcount + c), ~0ull);          // - 1
        const int64_t slot = tstart[c] + left - 1;
        if (left < 1 || slot >= m) return;                                                            // cannot be: the counts were made from the same cells
        tsorted[slot] = make_float4(target[3 * i], target[3 * i + 1], target[3 * i + 2], __int_as_float((int)i));
    } else if (i < m + n) {
        const int64_t q = i - m;
        const int c = qcell[q];
        if (c < 0) return;
        const int64_t left = (int64_t)atomicAdd((unsigned long long *)(qcount + c), ~0ull);
        const int64_t slot = qstart[c] + left - 1;
        if (left < 1 || slot >= n) return;
        qsorted[slot] = (int32_t)q;
        qsorted_cell[slot] = c;
    }
}

__global__ void __launch_bounds__(kThreads) cloud_nearest_kernel(const float *__restrict__ query, int64_t n, int64_t m, Cells G, float r_max,
                                                                 const int64_t *__restrict__ tstart, const int64_t *__restrict__ qstart,
                                                                 const float4 *__restrict__ tsorted, const int32_t *__restrict__ qsorted,
                                                                 const int32_t *__restrict__ qsorted_cell, int32_t *__restrict__ index, float *__restrict__ dist) {
    __shared__ float4 stage[kStage];
    const int64_t first = (int64_t)blockIdx.x * kThreads;
    int64_t listed = qstart[G.n];                       // the queries that are finite
    listed = listed < n ? listed : n;
    if (first >= listed) return;
    const int64_t end = first + kThreads < listed ? first + kThreads : listed;
    const int64_t slot = first + threadIdx.x;
    const bool have = slot < end;
    int my_cell = -1, my_query = 0;
    float qx = 0.0f, qy = 0.0f, qz = 0.0f;
    if (have) {
        my_query = qsorted[slot];
        my_cell = qsorted_cell[slot];
        qx = query[3 * (int64_t)my_query]; qy = query[3 * (int64_t)my_query + 1]; qz = query[3 * (int64_t)my_query + 2];
    }
    const float r2 = r_max * r_max;
    float best = r2;
    int best_i = 0x7fffffff;
    // the cells of this workgroup's queries, in order; each pass consumes at least one query, so at most kThreads passes
    for (int64_t cur = first; cur < end;) {
        const int cell = qsorted_cell[cur];
        if (cell < 0 || cell >= G.n) break;               // cannot be
        const int64_t cell_end = qstart[cell + 1];
        const bool mine = have && my_cell == cell;
        const int cz = cell % G.c[2], cy = (cell / G.c[2]) % G.c[1], cx = cell / (G.c[2] * G.c[1]);
        const int zlo = cz > 0 ? cz - 1 : 0, zhi = cz + 1 < G.c[2] ? cz + 1 : G.c[2] - 1;
        for (int dx = -1; dx <= 1; ++dx) {
            const int x = cx + dx;
            if (x < 0 || x >= G.c[0]) continue;
            for (int dy = -1; dy <= 1; ++dy) {
                const int y = cy + dy;
                if (y < 0 || y >= G.c[1]) continue;
                const int column = (x * G.c[1] + y) * G.c[2];
                int64_t run = tstart[column + zlo], run_end = tstart[column + zhi + 1];
                run_end = run_end < m ? run_end : m;
                for (; run < run_end; run += kStage) {
                    const int count = (int)(run_end - run < kStage ? run_end - run : kStage);
                    __syncthreads();                      // the last chunk is read
                    for (int k = threadIdx.x; k < count; k += kThreads) stage[k] = tsorted[run + k];
                    __syncthreads();
                    if (mine) {
#pragma unroll 4
                        for (int k = 0; k < count; ++k) {
                            const float4 t = stage[k];
                            const float ex = qx - t.x, ey = qy - t.y, ez = qz - t.z;
                            const float d2 = (ex * ex + ey * ey) + ez * ez;
                            const int ti = __float_as_int(t.w);
                            if (d2 < best || (d2 == best && ti < best_i)) { best = d2; best_i = ti; }
                        }
                    }
                }
            }
        }
        cur = cell_end > cur ? cell_end : cur + 1;        // cell_end > cur always; the guard only keeps the loop finite whatever the workspace holds
    }
    if (have) {
        const bool found = best_i != 0x7fffffff;
        index[my_query] = found ? best_i : -1;
        dist[my_query] = found ? sqrtf(best) : r_max;
    }
}

struct NearestWs { int64_t *tcount, *qcount, *tstart, *qstart, *scan; int32_t *tcell, *qcell, *qsorted, *qsorted_cell; float4 *tsorted; int64_t bytes; };

inline NearestWs carve_nearest(void *base, int64_t n, int64_t m, int64_t cells) {
    Carver c(base, 16);
    NearestWs w;
    w.tsorted = c.take<float4>(m);
    w.tcount = c.take<int64_t>(2 * cells);              // tcount and qcount side by side: one memset
    w.qcount = w.tcount ? w.tcount + cells : nullptr;
    w.tstart = c.take<int64_t>(cells + 1);
    w.qstart = c.take<int64_t>(cells + 1);
    w.tcell = c.take<int32_t>(m);
    w.qcell = c.take<int32_t>(n);
    w.qsorted = c.take<int32_t>(n);
    w.qsorted_cell = c.take<int32_t>(n);
    w.scan = (int64_t *)c.take(scan_bytes(cells));
    w.bytes = c.bytes();
    return w;
}

// ---------------------------------------------------------------------------------------------------------------- reduction
__global__ void __launch_bounds__(kThreads) cloud_stats_kernel(const float *__restrict__ dist, const int32_t *__restrict__ index, const float *__restrict__ query,
                                                               int64_t n, float thr, const int32_t *__restrict__ query_label,
                                                               const int32_t *__restrict__ target_label, int64_t m, int C, int64_t *__restrict__ counts,
                                                               double *__restrict__ sums, int64_t *__restrict__ confusion) {
    __shared__ double red_s[kThreads / 64][2];
    __shared__ unsigned long long red_c[kThreads / 64][3];
    unsigned long long c0 = 0, c1 = 0, c2 = 0;
    double s0 = 0.0, s1 = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads) {
        if (query) {
            const float x = query[3 * i], y = query[3 * i + 1], z = query[3 * i + 2];
            if (!(x - x == 0.0f && y - y == 0.0f && z - z == 0.0f)) continue;
        }
        const float d = dist[i];
        const int64_t j = index[i];
        const bool found = j >= 0 && j < m;
        c0 += 1;
        s0 += (double)d;
        if (!found) continue;
        c1 += 1;
        s1 += (double)d;
        if (!(d <= thr)) continue;
        c2 += 1;
        if (confusion) {
            const int a = query_label[i], b = target_label[j];
            if (a >= 0 && a < C && b >= 0 && b < C) atomicAdd((unsigned long long *)(confusion + (int64_t)a * C + b), 1ull);
        }
    }
    wave_sum_each(c0, c1, c2, s0, s1);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { red_c[wave][0] = c0; red_c[wave][1] = c1; red_c[wave][2] = c2; red_s[wave][0] = s0; red_s[wave][1] = s1; }
    __syncthreads();
    if (threadIdx.x < 3) {
        const int k = threadIdx.x;
        const unsigned long long v = (red_c[0][k] + red_c[1][k]) + (red_c[2][k] + red_c[3][k]);
        if (v) atomicAdd((unsigned long long *)(counts + k), v);
    } else if (threadIdx.x >= 64 && threadIdx.x < 66) {
        const int k = threadIdx.x - 64;
        atomicAdd(sums + k, (red_s[0][k] + red_s[1][k]) + (red_s[2][k] + red_s[3][k]));
    }
}

}  // namespace
}  // namespace mnf

using namespace mnf;

extern "C" int64_t mnf_cloud_sample_triangles_workspace_bytes(int64_t n_triangles, int64_t max_rows) {
    if (!sample_sizes_ok(n_triangles, max_rows)) return 0;
    return carve_sample(nullptr, n_triangles, max_rows).bytes;
}

extern "C" int mnf_cloud_sample_triangles(const float *positions, int64_t n_vertices, const int32_t *triangles, int64_t n_triangles, double res,
                                          int64_t max_rows, int64_t max_points, float *points, int32_t *face, int64_t *info, void *workspace,
                                          int64_t workspace_bytes, mnf_stream_t stream) {
    MNF_REQUIRE(n_vertices >= 0 && n_vertices <= kMaxCount, "cloud_sample_triangles: n_vertices outside [0, 2^31) (got %lld)", (long long)n_vertices);
    MNF_REQUIRE(n_triangles >= 0 && n_triangles <= kMaxCount, "cloud_sample_triangles: n_triangles outside [0, 2^31) (got %lld)", (long long)n_triangles);
    MNF_REQUIRE(res > 0.0 && finite_d(res), "cloud_sample_triangles: res must be positive and finite (got %g)", res);
    MNF_REQUIRE(max_rows >= 0 && max_rows <= kMaxCount, "cloud_sample_triangles: max_rows outside [0, 2^31) (got %lld)", (long long)max_rows);
    MNF_REQUIRE(max_points >= 0 && max_points <= kMaxCount, "cloud_sample_triangles: max_points outside [0, 2^31) (got %lld)", (long long)max_points);
    MNF_REQUIRE(positions || n_vertices == 0, "cloud_sample_triangles: positions is null");
    MNF_REQUIRE(triangles || n_triangles == 0, "cloud_sample_triangles: triangles is null");
    MNF_REQUIRE(points || max_points == 0, "cloud_sample_triangles: points is null");
    MNF_REQUIRE(face || max_points == 0, "cloud_sample_triangles: face is null");
    MNF_REQUIRE(info, "cloud_sample_triangles: info is null");
    MNF_REQUIRE(aligned8(info), "cloud_sample_triangles: info must be 8-byte aligned");
    MNF_REQUIRE(workspace, "cloud_sample_triangles: workspace is null");
    MNF_REQUIRE(aligned8(workspace), "cloud_sample_triangles: workspace must be 8-byte aligned");
    const SampleWs w = carve_sample(workspace, n_triangles, max_rows);
    MNF_REQUIRE(workspace_bytes >= w.bytes, "cloud_sample_triangles: workspace too small (%lld < %lld bytes)", (long long)workspace_bytes, (long long)w.bytes);
    hipStream_t s = as_stream(stream);
    ProfScope prof("cloud_sample_triangles", s);
    const int64_t T = n_triangles;
    int rc;
    if (T > 0) {
        hipLaunchKernelGGL(cloud_tri_rows_kernel, dim3(blocks_for(T)), dim3(kThreads), 0, s, positions, n_vertices, triangles, T, res, w.tri_rows);
        rc = launch_status("cloud_tri_rows_kernel");
        if (rc) return rc;
    }
    rc = mnf_exclusive_scan_i64(w.tri_rows, T, w.tri_base, w.totals, w.scan, scan_bytes(T), stream);
    if (rc) return rc;
    if (max_rows > 0 && T > 0) {
        hipLaunchKernelGGL(cloud_row_points_kernel, dim3(blocks_for(max_rows)), dim3(kThreads), 0, s, positions, n_vertices, triangles, T, res, w.tri_base,
                           w.totals, max_rows, w.row_tri, w.row_points);
        rc = launch_status("cloud_row_points_kernel");
        if (rc) return rc;
        rc = mnf_exclusive_scan_i64(w.row_points, max_rows, w.row_base, w.totals + 1, w.scan, scan_bytes(max_rows), stream);
        if (rc) return rc;
    }
    hipLaunchKernelGGL(cloud_fill_kernel, dim3(blocks_for(max_points)), dim3(kThreads), 0, s, positions, n_vertices, triangles, res, w.tri_base, w.totals,
                       T > 0 ? max_rows : 0, w.row_tri, w.row_base, w.totals + 1, max_points, points, face, info);
    return launch_status("cloud_fill_kernel");
}

extern "C" int64_t mnf_cloud_nearest_workspace_bytes(int64_t n, int64_t m, const float *box_host, float r_max) {
    Cells G;
    if (n < 0 || n > kMaxCount || m < 0 || m > kMaxCount || !make_cells(box_host, r_max, &G)) return 0;
    return carve_nearest(nullptr, n, m, G.n).bytes;
}

extern "C" int mnf_cloud_nearest(const float *query, int64_t n, const float *target, int64_t m, float r_max, const float *box_host, int32_t *index, float *dist,
                                 void *workspace, int64_t workspace_bytes, mnf_stream_t stream) {
    Cells G;
    MNF_REQUIRE(n >= 0 && n <= kMaxCount, "cloud_nearest: n outside [0, 2^31) (got %lld)", (long long)n);
    MNF_REQUIRE(m >= 0 && m <= kMaxCount, "cloud_nearest: m outside [0, 2^31) (got %lld)", (long long)m);
    MNF_REQUIRE(radius_ok(r_max), "cloud_nearest: r_max must be at least 2^-60 with a finite square (got %g)", (double)r_max);
    MNF_REQUIRE(box_host, "cloud_nearest: box is null");
    MNF_REQUIRE(make_cells(box_host, r_max, &G), "cloud_nearest: the box must be finite with max >= min on every axis");
    MNF_REQUIRE(query || n == 0, "cloud_nearest: query is null");
    MNF_REQUIRE(target || m == 0, "cloud_nearest: target is null");
    MNF_REQUIRE(index || n == 0, "cloud_nearest: index is null");
    MNF_REQUIRE(dist || n == 0, "cloud_nearest: dist is null");
    MNF_REQUIRE(workspace, "cloud_nearest: workspace is null");
    MNF_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 15) == 0, "cloud_nearest: workspace must be 16-byte aligned");
    const NearestWs w = carve_nearest(workspace, n, m, G.n);
    MNF_REQUIRE(workspace_bytes >= w.bytes, "cloud_nearest: workspace too small (%lld < %lld bytes)", (long long)workspace_bytes, (long long)w.bytes);
    if (n == 0) return MNF_OK;
    hipStream_t s = as_stream(stream);
    ProfScope prof("cloud_nearest", s);
    MNF_HIP(hipMemsetAsync(w.tcount, 0, (size_t)(2 * G.n) * sizeof(int64_t), s));
    hipLaunchKernelGGL(cloud_bin_kernel, dim3(blocks_for(n + m)), dim3(kThreads), 0, s, query, n, target, m, G, r_max, w.tcell, w.qcell, w.tcount, w.qcount, index,
                       dist);
    int rc = launch_status("cloud_bin_kernel");
    if (rc) return rc;
    rc = mnf_exclusive_scan_i64(w.tcount, G.n, w.tstart, w.tstart + G.n, w.scan, scan_bytes(G.n), stream);
    if (rc) return rc;
    rc = mnf_exclusive_scan_i64(w.qcount, G.n, w.qstart, w.qstart + G.n, w.scan, scan_bytes(G.n), stream);
    if (rc) return rc;
    hipLaunchKernelGGL(cloud_place_kernel, dim3(blocks_for(n + m)), dim3(kThreads), 0, s, target, n, m, w.tcell, w.qcell, w.tstart, w.qstart, w.tcount, w.qcount,
                       w.tsorted, w.qsorted, w.qsorted_cell);
    rc = launch_status("cloud_place_kernel");
    if (rc) return rc;
    hipLaunchKernelGGL(cloud_nearest_kernel, dim3(blocks_for(n)), dim3(kThreads), 0, s, query, n, m, G, r_max, w.tstart, w.qstart, w.tsorted, w.qsorted,
                       w.qsorted_cell, index, dist);
    return launch_status("cloud_nearest_kernel");
}

extern "C" int mnf_cloud_distance_stats(const float *dist, const int32_t *index, const float *query, int64_t n, float thr, float r_max,
                                        const int32_t *query_label, const int32_t *target_label, int64_t m, int32_t n_classes, int64_t *counts, double *sums,
                                        int64_t *confusion, mnf_stream_t stream) {
    MNF_REQUIRE(n >= 0 && n <= kMaxCount, "cloud_distance_stats: n outside [0, 2^31) (got %lld)", (long long)n);
    MNF_REQUIRE(m >= 0 && m <= kMaxCount, "cloud_distance_stats: m outside [0, 2^31) (got %lld)", (long long)m);
    MNF_REQUIRE(r_max > 0.0f && finite_f(r_max), "cloud_distance_stats: r_max must be positive and finite (got %g)", (double)r_max);
    MNF_REQUIRE(thr >= 0.0f && thr <= r_max, "cloud_distance_stats: thr must lie in [0, r_max] (got %g, r_max %g)", (double)thr, (double)r_max);
    MNF_REQUIRE(dist || n == 0, "cloud_distance_stats: dist is null");
    MNF_REQUIRE(index || n == 0, "cloud_distance_stats: index is null");
    MNF_REQUIRE(counts, "cloud_distance_stats: counts is null");
    MNF_REQUIRE(sums, "cloud_distance_stats: sums is null");
    MNF_REQUIRE(aligned8(counts) && aligned8(sums) && aligned8(confusion), "cloud_distance_stats: counts, sums and confusion must be 8-byte aligned");
    if (confusion) {
        MNF_REQUIRE(n_classes >= 1 && n_classes <= kMaxClasses, "cloud_distance_stats: n_classes outside 1 .. %d (got %d)", kMaxClasses, n_classes);
        MNF_REQUIRE(query_label || n == 0, "cloud_distance_stats: confusion asks for query_label");
        MNF_REQUIRE(target_label || m == 0, "cloud_distance_stats: confusion asks for target_label");
    }
    hipStream_t s = as_stream(stream);
    ProfScope prof("cloud_distance_stats", s);
    MNF_HIP(hipMemsetAsync(counts, 0, 3 * sizeof(int64_t), s));
    MNF_HIP(hipMemsetAsync(sums, 0, 2 * sizeof(double), s));
    if (confusion) MNF_HIP(hipMemsetAsync(confusion, 0, (size_t)n_classes * n_classes * sizeof(int64_t), s));
    if (n == 0) return MNF_OK;
    const unsigned nb = blocks_for(n) < 1024u ? blocks_for(n) : 1024u;
    hipLaunchKernelGGL(cloud_stats_kernel, dim3(nb), dim3(kThreads), 0, s, dist, index, query, n, thr, query_label, target_label, m, confusion ? n_classes : 0,
                       counts, sums, confusion);
    return launch_status("cloud_stats_kernel");
}
