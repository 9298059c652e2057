// Min-snap candidate trajectories on the device (gfx950): the curve through a traced path, its samples, and the view poses of the samples.
//   mnf_minsnap_solve         <- planning/rotorpy/rotorpy/trajectories/minsnap.py:254-371 (MinSnap.__init__, initialize) with the waypoints of
//                                planning/planning_funcs.py:328-343 (sample_traj: the reversed path, index * resolution + aabb, the yaw sweep)
//   mnf_minsnap_sample_count  <- planning/planning_funcs.py:352-370 (t_final, N_sample_disc, t_step, the running sum of sample times, time_exit)
//   mnf_minsnap_sample_fill   <- minsnap.py:386-443 (update), controllers/quadrotor_control.py:104-124, :177 (update_ref's attitude and cmd_q),
//                                planning_funcs.py:377-395 (the x, z, y position, the axis shuffle of cmd_q, the look-around poses)
// Built with -ffp-contract=off.  Everything is float64.  The time allocation, the keyframe times, the sample times and the sample counts are
// chains of separately rounded + - * / sqrt in the reference's order, np.sum's pairwise order included; the coefficients are the solution of
// the reference's square system A c = b by another elimination order, so they agree with it to rounding, not bit for bit.
//
// The system.  For m segments the unknowns are c[8 i + k], the coefficient of t^k of segment i.  With the rows ordered
//   0..2                    velocity, acceleration, jerk = 0 at the start
//   3 + 8 i, 4 + 8 i        segment i passes through keyframe i at 0 and keyframe i + 1 at dt_i
//   4 + 8 i + d, d = 1..6   derivative d is continuous from segment i to i + 1                       (i < m - 1)
//   8 m - 3 .. 8 m - 1      velocity, acceleration, jerk = 0 at the end
// A has lower and upper bandwidth 4 whatever m is, and is the same matrix for x, y, z and yaw.  solve_kernel, one wave per trajectory:
// Gaussian elimination with partial pivoting over the five rows that can hold the pivot of a column, nine columns wide after fill-in, with the
// four right-hand sides beside them.  Only that window lives in LDS (a band entry of column c sits in word c & 15 of its row's slot; words
// outside the nine live columns are kept zero).  The 48 multiply-subtracts of a step go to 48 lanes, 13 more lanes write the pivot row to the
// caller's workspace, and the freed slot takes the next row, which is assembled in closed form from dt.  Back substitution reads the factored
// rows back through LDS, 32 at a time, one lane per right-hand side.  Partial pivoting because the rows mix 1, dt^7 and 5040 dt: with dt from
// 0.4 s to a few seconds the natural pivots span eight orders of magnitude and elimination without row exchanges loses the curve.
// A pivot below n eps |A|_inf (n = 8 m) ends the trajectory with MNF_MINSNAP_SINGULAR: this project's criterion, not the reference's rank test.
#include "common.h"

namespace mnf {
namespace {

constexpr int kMaxSeg = MNF_MINSNAP_MAX_SEGMENTS;
constexpr int kMaxWaypoints = 4096;                   // of one trajectory, before the mask (np.sum's pairwise tree below is six levels deep)
constexpr int kRow = 13;                              // a factored row: the pivot and eight entries right of it, four right-hand sides
constexpr int kChunk = 32;                            // factored rows per LDS load of the back substitution
constexpr double kEps = 2.220446049250313e-16;
constexpr double kG = 9.81;                           // SE3Control.g

inline int64_t solve_workspace_bytes(int64_t n_waypoints) { return n_waypoints * (int64_t)(8 + 8 * kRow * 8); }

// np.sum of a contiguous float64 array (numpy's pairwise sum: plain below 8, eight accumulators up to 128, halves rounded to 8 above)
__device__ double np_sum_block(const double *a, int n) {
    if (n < 8) {
        double res = 0.0;
        for (int i = 0; i < n; ++i) res += a[i];
        return res;
    }
    double r[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) r[k] = a[k];
    int i;
    for (i = 8; i < n - (n % 8); i += 8) {
#pragma unroll
        for (int k = 0; k < 8; ++k) r[k] += a[i + k];
    }
    double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; ++i) res += a[i];
    return res;
}

template <int kDepth>
__device__ double np_sum(const double *a, int n) {
    if (n <= 128) return np_sum_block(a, n);
    int n2 = n / 2;
    n2 -= n2 % 8;
    if constexpr (kDepth > 0) return np_sum<kDepth - 1>(a, n2) + np_sum<kDepth - 1>(a + n2, n - n2);
    else return np_sum_block(a, n);                   // not reached: n <= kMaxWaypoints
}

// k! / (k - d)!
__device__ __forceinline__ double falling(int k, int d) {
    double f = 1.0;
    for (int q = 0; q < d; ++q) f *= (double)(k - q);
    return f;
}

__device__ __forceinline__ double power(double dt, int e) {
    double p = 1.0;
    for (int q = 0; q < e; ++q) p *= dt;
    return p;
}

// A[r][col] of the reordered system
__device__ double band_entry(int r, int col, int m, const double *dts) {
    if (col < 0 || col >= 8 * m) return 0.0;
    if (r < 3) return col == r + 1 ? falling(r + 1, r + 1) : 0.0;
    const int q = r - 3, i = q >> 3, j = q & 7;
    const int k = col - 8 * i;
    if (j == 0) return k == 0 ? 1.0 : 0.0;
    if (j == 1) return (k >= 0 && k <= 7) ? power(dts[i], k) : 0.0;
    const int d = j - 1;
    if (i == m - 1) return (k >= d && k <= 7) ? falling(k, d) * power(dts[i], k - d) : 0.0;         // d = 1, 2, 3: the end rows
    if (k >= d && k <= 7) return -(falling(k, d) * power(dts[i], k - d));
    return k == 8 + d ? falling(d, d) : 0.0;
}

// b[r] for axis a (0, 1, 2 the position, 3 the yaw)
__device__ __forceinline__ double rhs_entry(int r, int a, const double *kp, const double *yawx) {
    if (r < 3) return 0.0;
    const int q = r - 3, i = q >> 3, j = q & 7;
    if (j > 1) return 0.0;
    return a < 3 ? kp[3 * (i + j) + a] : yawx[i + j];
}

__device__ __forceinline__ bool finite3(double x, double y, double z) { return isfinite(x) && isfinite(y) && isfinite(z); }

__global__ void __launch_bounds__(64) solve_kernel(const double *__restrict__ points, const int32_t *__restrict__ cells, const int64_t *__restrict__ offsets,
                                                   int64_t n_waypoints, double resolution, double ox, double oy, double oz, double height, double yaw0,
                                                   double yaw1, double v_avg, double *__restrict__ coeffs, double *__restrict__ delta_t,
                                                   double *__restrict__ t_keyframes, double *__restrict__ yaw_execute, int32_t *__restrict__ n_segments,
                                                   int32_t *__restrict__ status, double *__restrict__ ws_dist, double *__restrict__ ws_rows) {
    __shared__ double sd[kMaxSeg + 1];                // seg_dist[0 .. m), later yaw_execute[0 .. m]
    __shared__ double dts[kMaxSeg + 1];
    __shared__ double tks[kMaxSeg + 1];
    __shared__ double kp[3 * (kMaxSeg + 1)];
    __shared__ double win[5][16];
    __shared__ double rwin[5][4];
    __shared__ double chunk[kChunk * kRow];
    const int lane = threadIdx.x;
    const int64_t t = blockIdx.x;
    int64_t w0 = offsets[t], w1 = offsets[t + 1];
    w0 = w0 < 0 ? 0 : w0 > n_waypoints ? n_waypoints : w0;
    w1 = w1 < w0 ? w0 : w1 > n_waypoints ? n_waypoints : w1;
    const int64_t Wl = w1 - w0;
    if (Wl <= 0) { if (lane == 0) { status[t] = MNF_MINSNAP_NULL; n_segments[t] = 0; } return; }
    if (Wl > kMaxWaypoints) { if (lane == 0) { status[t] = MNF_MINSNAP_TOO_LONG; n_segments[t] = 0; } return; }
    const int W = (int)Wl;
    auto waypoint = [&](int k, double &x, double &y, double &z) {
        if (points) {
            const double *p = points + 3 * (w0 + k);
            x = p[0]; y = p[1]; z = p[2];
        } else {                                      // trace_paths lists the goal first: reversed, index * resolution + aabb as sample_traj forms it
            const int32_t *c = cells + 2 * (w1 - 1 - k);
            x = (double)c[0] * resolution + ox; y = (double)c[1] * resolution + oy; z = height + oz;
        }
    };
    // seg_dist over ALL waypoints, seg_mask, the kept points
    int kept = 0;
    bool bad = false;
    for (int base = 0; base < W; base += 64) {
        const int k = base + lane;
        bool keep = false;
        double x = 0.0, y = 0.0, z = 0.0;
        if (k < W) {
            waypoint(k, x, y, z);
            bad = bad || !finite3(x, y, z);
            keep = true;
            if (k > 0) {
                double px, py, pz;
                waypoint(k - 1, px, py, pz);
                const double dx = x - px, dy = y - py, dz = z - pz;
                const double d = sqrt((dx * dx + dy * dy) + dz * dz);
                ws_dist[w0 + k - 1] = d;
                if (k - 1 <= kMaxSeg) sd[k - 1] = d;
                keep = d > 1e-2;
            }
        }
        const unsigned long long votes = __ballot(keep);
        if (keep) {
            const int at = kept + __popcll(votes & ((1ull << lane) - 1ull));
            if (at <= kMaxSeg) { kp[3 * at] = x; kp[3 * at + 1] = y; kp[3 * at + 2] = z; }
        }
        kept += __popcll(votes);
    }
    const int m = kept - 1;
    int st = MNF_MINSNAP_OK;
    if (__ballot(bad)) st = MNF_MINSNAP_NOT_FINITE;
    else if (m == 0) st = MNF_MINSNAP_NULL;
    else if (m == 1) st = MNF_MINSNAP_REJECTED_SHORT;
    else if (m > kMaxSeg) st = MNF_MINSNAP_TOO_LONG;
    if (st != MNF_MINSNAP_OK) { if (lane == 0) { status[t] = st; n_segments[t] = m; } return; }
    __syncthreads();
    // the time allocation: one lane, the reference's recurrence
    if (lane == 0) {
        const double total = np_sum<6>(ws_dist + w0, W - 1);
        double vi = 0.0, cum = 0.0, tk = 0.0;
        tks[0] = 0.0;
        for (int i = 0; i < m; ++i) {
            cum += sd[i];
            const double a = v_avg < cum ? v_avg : cum;                               // min(cum_dist, v_avg)
            const double rest = total - cum;
            const double vf = rest < a ? rest : a;
            const double dt = sd[i] * 2.0 / ((vf + vi) + 1e-4);
            dts[i] = dt;
            vi = vf;
            tk += dt;
            tks[i + 1] = tk;
        }
    }
    __syncthreads();
    const double T_end = tks[m];
    const double yaw_diff = yaw1 - yaw0;
    bool odd = false;
    for (int i = lane; i <= m; i += 64) {
        const double ye = tks[i] / (T_end + 1e-4) * yaw_diff + yaw0;
        odd = odd || !isfinite(ye) || (i < m && !(dts[i] > 0.0 && isfinite(dts[i])));
        sd[i] = ye;
    }
    __syncthreads();
    const double *yawx = sd;
    const int n = 8 * m;
    // |A|_inf
    double norm = 0.0;
    for (int r = lane; r < n; r += 64) {
        double s = 0.0;
        for (int c = r - 4; c <= r + 4; ++c) s += fabs(band_entry(r, c, m, dts));
        norm = s > norm ? s : norm;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { const double o = __shfl_xor(norm, off, 64); norm = o > norm ? o : norm; }
    const double thresh = (double)n * kEps * norm;
    bool singular = __ballot(odd) != 0ull || !isfinite(norm);
    double *rows = ws_rows + (int64_t)8 * w0 * kRow;                                  // n <= 8 (W - 1) rows of this trajectory
    // the first five rows
    auto load_row = [&](int slot, int r) {                                            // lanes 0..15 the band words, 16..19 the right-hand sides
        if (lane < 16) {
            const int col = r - 4 + ((lane - (r - 4)) & 15);
            win[slot][lane] = (r < n && col <= r + 4) ? band_entry(r, col, m, dts) : 0.0;
        } else if (lane < 20) {
            rwin[slot][lane - 16] = r < n ? rhs_entry(r, lane - 16, kp, yawx) : 0.0;
        }
    };
    if (!singular) {
        for (int s = 0; s < 5; ++s) load_row(s, s);
    }
    __syncthreads();
    for (int j = 0; j < n && !singular; ++j) {
        const int cj = j & 15;
        double v[5];
#pragma unroll
        for (int s = 0; s < 5; ++s) v[s] = win[s][cj];
        int p = 0;
        double best = fabs(v[0]);
#pragma unroll
        for (int s = 1; s < 5; ++s) { const double a = fabs(v[s]); if (a > best) { best = a; p = s; } }
        if (!(best >= thresh) || !(best > 0.0)) { singular = true; break; }         // uniform: every lane reads the same five words
        const double piv = v[p];
        if (lane < 48) {
            const int q = lane / 12, c = lane - 12 * q;
            const int slot = q + (q >= p ? 1 : 0);
            const double l = v[slot] / piv;
            if (c < 8) {
                const int w = (j + 1 + c) & 15;
                win[slot][w] = win[slot][w] - l * win[p][w];
            } else {
                rwin[slot][c - 8] = rwin[slot][c - 8] - l * rwin[p][c - 8];
            }
        } else if (lane < 48 + kRow) {
            const int c = lane - 48;
            rows[(int64_t)j * kRow + c] = c < 9 ? win[p][(j + c) & 15] : rwin[p][c - 9];
        }
        __syncthreads();
        if (lane < 5 && lane != p) win[lane][cj] = 0.0;                               // column j is eliminated: its word stands for column j + 16 next
        load_row(p, j + 5);                                                           // a row past the end is all zeros and never wins a pivot
        __syncthreads();
    }
    if (singular) { if (lane == 0) { status[t] = MNF_MINSNAP_SINGULAR; n_segments[t] = m; } return; }
    // back substitution, the last chunk first
    double x[8];                                                                      // x[c] = the unknown c + 1 places right of the current one
#pragma unroll
    for (int c = 0; c < 8; ++c) x[c] = 0.0;
    double *out = coeffs + (int64_t)w0 * 32;
    bool nonfinite = false;
    for (int hi = n; hi > 0; hi -= kChunk) {
        const int lo = hi - kChunk > 0 ? hi - kChunk : 0;
        __syncthreads();
        for (int e = lane; e < (hi - lo) * kRow; e += 64) chunk[e] = rows[(int64_t)lo * kRow + e];
        __syncthreads();
        if (lane < 4) {
            for (int j = hi - 1; j >= lo; --j) {
                const double *u = chunk + (j - lo) * kRow;
                double acc = u[9 + lane];
#pragma unroll
                for (int c = 0; c < 8; ++c) acc -= u[1 + c] * x[c];
                const double xj = acc / u[0];
#pragma unroll
                for (int c = 7; c > 0; --c) x[c] = x[c - 1];
                x[0] = xj;
                nonfinite = nonfinite || !isfinite(xj);
                out[(int64_t)(j >> 3) * 32 + lane * 8 + (j & 7)] = xj;
            }
        }
    }
    const bool any_bad = __ballot(nonfinite) != 0ull;
    for (int i = lane; i <= m; i += 64) {
        if (i < m) delta_t[w0 + i] = dts[i];
        t_keyframes[w0 + i] = tks[i];
        yaw_execute[w0 + i] = yawx[i];
    }
    if (lane == 0) { status[t] = any_bad ? MNF_MINSNAP_SINGULAR : MNF_MINSNAP_OK; n_segments[t] = m; }
}

// one lane per trajectory: the sample times as the reference's loop forms them
__global__ void __launch_bounds__(64) sample_count_kernel(const double *__restrict__ delta_t, const int64_t *__restrict__ offsets, int64_t n_waypoints,
                                                          const int32_t *__restrict__ n_segments, const int32_t *__restrict__ status, int64_t n_traj, double rate,
                                                          long long min_samples, long long max_samples, long long *__restrict__ counts,
                                                          int32_t *__restrict__ sample_status, double *__restrict__ ws_times) {
    const int64_t t = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (t >= n_traj) return;
    counts[t] = 0;
    sample_status[t] = 0;
    if (status[t] != MNF_MINSNAP_OK) return;
    const int64_t w0 = offsets[t];
    const int m = n_segments[t];
    if (m < 1 || m > kMaxSeg || w0 < 0 || w0 + m > n_waypoints) { sample_status[t] = MNF_MINSNAP_SAMPLE_INVALID; return; }
    const double t_final = np_sum<6>(delta_t + w0, m);
    const double scaled = t_final * rate;
    if (!(scaled < 1099511627776.0)) { sample_status[t] = MNF_MINSNAP_SAMPLE_OVERFLOW; return; }     // NaN included
    long long N = (long long)scaled;                                                  // int() truncates
    N = N > min_samples ? N : min_samples;                                            // max(int(t_final * rate), min_samples)
    const double t_step = t_final / (double)N;
    double *times = ws_times + t * max_samples;
    double time = 0.0;
    long long c = 0;
    for (;;) {
        if (c >= max_samples) { sample_status[t] = MNF_MINSNAP_SAMPLE_OVERFLOW; return; }
        times[c++] = time;
        if (time >= t_final) break;                                                   // time_exit
        time = time + t_step;
    }
    counts[t] = c;
}

struct Flat { double x[3], d1[3], d2[3], d3[3], d4[3], yaw, yaw_dot, yaw_ddot; };

// np.polyval of the derivative `order` of a segment's polynomial c[0..7] (lowest power first), the coefficients formed as np.polyder forms them:
// one multiplication by an integer per order
__device__ __forceinline__ double poly_eval(const double *__restrict__ c, int order, double tau) {
    double y = 0.0;
    bool first = true;
    for (int k = 7; k >= order; --k) {
        double pv = c[k];
        for (int q = 0; q < order; ++q) pv = pv * (double)(k - q);
        y = first ? pv : y * tau + pv;
        first = false;
    }
    return y;
}

__device__ void evaluate(const double *__restrict__ coeffs, const double *__restrict__ dts, const double *__restrict__ tks, int m, double time, bool all,
                         Flat *f) {
    const double lo = tks[0], hi = tks[m];
    double tc = time < lo ? lo : time;                                                // np.clip
    tc = tc > hi ? hi : tc;
    int a = 0, b = m - 1;                                                             // the first i with t_keyframes[i] + delta_t[i] >= t, else m - 1
    while (a < b) {
        const int mid = (a + b) >> 1;
        if (tks[mid] + dts[mid] >= tc) b = mid; else a = mid + 1;
    }
    const double tau = tc - tks[a];
    const double *c = coeffs + (int64_t)a * 32;
    for (int j = 0; j < 3; ++j) {
        f->x[j] = poly_eval(c + 8 * j, 0, tau);
        f->d2[j] = poly_eval(c + 8 * j, 2, tau);
        if (all) { f->d1[j] = poly_eval(c + 8 * j, 1, tau); f->d3[j] = poly_eval(c + 8 * j, 3, tau); f->d4[j] = poly_eval(c + 8 * j, 4, tau); }
    }
    f->yaw = poly_eval(c + 24, 0, tau);
    if (all) { f->yaw_dot = poly_eval(c + 24, 1, tau); f->yaw_ddot = poly_eval(c + 24, 2, tau); }
}

// update_ref's R_des, scipy's Rotation.from_matrix(R_des).as_quat(), and sample_traj's from_rotvec(P as_rotvec(q)) in closed form
__device__ void attitude(const Flat &f, double *q) {
    const double tx = f.d2[0] + 0.0, ty = f.d2[1] + 0.0, tz = f.d2[2] + kG;
    const double tn = sqrt((tx * tx + ty * ty) + tz * tz);
    const double b3[3] = {tx / tn, ty / tn, tz / tn};
    const double c1[3] = {cos(f.yaw), sin(f.yaw), 0.0};
    double b2[3] = {b3[1] * c1[2] - b3[2] * c1[1], b3[2] * c1[0] - b3[0] * c1[2], b3[0] * c1[1] - b3[1] * c1[0]};
    const double n2 = sqrt((b2[0] * b2[0] + b2[1] * b2[1]) + b2[2] * b2[2]);
    b2[0] /= n2; b2[1] /= n2; b2[2] /= n2;
    const double b1[3] = {b2[1] * b3[2] - b2[2] * b3[1], b2[2] * b3[0] - b2[0] * b3[2], b2[0] * b3[1] - b2[1] * b3[0]};
    // R[r][c]: column 0 = b1, 1 = b2, 2 = b3
    const double R[3][3] = {{b1[0], b2[0], b3[0]}, {b1[1], b2[1], b3[1]}, {b1[2], b2[2], b3[2]}};
    const double trace = (R[0][0] + R[1][1]) + R[2][2];
    const double dec[4] = {R[0][0], R[1][1], R[2][2], trace};
    int choice = 0;
    for (int k = 1; k < 4; ++k) if (dec[k] > dec[choice]) choice = k;
    double u[4];
    if (choice != 3) {
        const int i = choice, j = (i + 1) % 3, k = (j + 1) % 3;
        u[i] = 1.0 - trace + 2.0 * R[i][i];
        u[j] = R[j][i] + R[i][j];
        u[k] = R[k][i] + R[i][k];
        u[3] = R[k][j] - R[j][k];
    } else {
        u[0] = R[2][1] - R[1][2];
        u[1] = R[0][2] - R[2][0];
        u[2] = R[1][0] - R[0][1];
        u[3] = 1.0 + trace;
    }
    const double un = sqrt(((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2]) + u[3] * u[3]);
    const double s = u[3] < 0.0 ? -1.0 : 1.0;                                         // as_rotvec takes the quaternion with w >= 0
    q[0] = -(s * (u[0] / un));
    q[1] = s * (u[2] / un);
    q[2] = -(s * (u[1] / un));
    q[3] = s * (u[3] / un);
}

// one thread per pose row
__global__ void __launch_bounds__(256) sample_fill_kernel(const double *__restrict__ coeffs, const double *__restrict__ delta_t, const double *__restrict__ t_keyframes,
                                                          const int64_t *__restrict__ offsets, int64_t n_waypoints, const int32_t *__restrict__ n_segments,
                                                          int64_t n_traj, int64_t max_samples, const int64_t *__restrict__ sample_offsets, int64_t n_samples,
                                                          const int64_t *__restrict__ pose_offsets, int64_t n_poses, const double *__restrict__ look_quats,
                                                          int n_look, double *__restrict__ flat_x, double *__restrict__ times_out, double *__restrict__ derivs,
                                                          double *__restrict__ yaw_out, double *__restrict__ poses, const double *__restrict__ ws_times) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n_poses) return;
    int64_t a = 0, b = n_traj - 1;                                                    // the last trajectory with pose_offsets[t] <= p
    while (a < b) {
        const int64_t mid = (a + b + 1) >> 1;
        if (pose_offsets[mid] <= p) a = mid; else b = mid - 1;
    }
    const int64_t t = a;
    const int64_t p0 = pose_offsets[t], p1 = pose_offsets[t + 1], s0 = sample_offsets[t], s1 = sample_offsets[t + 1];
    const int64_t S = s1 - s0;
    // a slot that is not the one the count pass sized is left alone
    if (p < p0 || p >= p1 || S <= 0 || S > max_samples || p1 - p0 != S + n_look || s0 < 0 || s1 > n_samples || p1 > n_poses) return;
    const int64_t w0 = offsets[t];
    const int m = n_segments[t];
    if (m < 1 || m > kMaxSeg || w0 < 0 || w0 + m + 1 > n_waypoints) return;
    const int64_t k = p - p0;
    const bool look = k >= S;
    const int64_t ks = look ? S - 1 : k;
    const double time = ws_times[t * max_samples + ks];
    Flat f;
    evaluate(coeffs + w0 * 32, delta_t + w0, t_keyframes + w0, m, time, !look && (derivs != nullptr || yaw_out != nullptr), &f);
    double *row = poses + 7 * p;
    row[0] = f.x[0]; row[1] = f.x[2]; row[2] = f.x[1];                                // xzy_x
    if (look) {
        const double *q = look_quats + 4 * (k - S);
        row[3] = q[0]; row[4] = q[1]; row[5] = q[2]; row[6] = q[3];
        return;
    }
    double q[4];
    attitude(f, q);
    row[3] = q[0]; row[4] = q[1]; row[5] = q[2]; row[6] = q[3];
    const int64_t s = s0 + k;
    flat_x[3 * s] = f.x[0]; flat_x[3 * s + 1] = f.x[1]; flat_x[3 * s + 2] = f.x[2];
    times_out[s] = time;
    if (derivs) {
        double *d = derivs + 12 * s;
        for (int j = 0; j < 3; ++j) { d[j] = f.d1[j]; d[3 + j] = f.d2[j]; d[6 + j] = f.d3[j]; d[9 + j] = f.d4[j]; }
    }
    if (yaw_out) { yaw_out[3 * s] = f.yaw; yaw_out[3 * s + 1] = f.yaw_dot; yaw_out[3 * s + 2] = f.yaw_ddot; }
}

}  // namespace
}  // namespace mnf

using namespace mnf;

extern "C" int64_t mnf_minsnap_workspace_bytes(int64_t n_traj, int64_t n_waypoints, int64_t max_samples) {
    if (n_traj < 0 || n_waypoints < 0 || max_samples < 0 || n_traj >= ((int64_t)1 << 31) || n_waypoints >= ((int64_t)1 << 31) || max_samples >= ((int64_t)1 << 31))
        return -1;
    const int64_t solve = solve_workspace_bytes(n_waypoints), sample = n_traj * max_samples * 8;
    const int64_t need = solve > sample ? solve : sample;
    return need > 8 ? need : 8;
}

extern "C" int mnf_minsnap_solve(const double *points, const int32_t *cells, const int64_t *offsets, int64_t n_traj, int64_t n_waypoints, double resolution,
                                 const double *origin_host, double height, double yaw0, double yaw1, double v_avg, double *coeffs, double *delta_t,
                                 double *t_keyframes, double *yaw_execute, int32_t *n_segments, int32_t *status, void *workspace, int64_t workspace_bytes,
                                 mnf_stream_t stream) {
    MNF_REQUIRE(n_traj >= 0 && n_traj < ((int64_t)1 << 31), "minsnap_solve: n_traj outside [0, 2^31) (%lld)", (long long)n_traj);
    MNF_REQUIRE(n_waypoints >= 0 && n_waypoints < ((int64_t)1 << 31), "minsnap_solve: n_waypoints outside [0, 2^31) (%lld)", (long long)n_waypoints);
    MNF_REQUIRE((points != nullptr) != (cells != nullptr) || n_waypoints == 0, "minsnap_solve: give points or cells, one of the two");
    MNF_REQUIRE(finite_d(yaw0) && finite_d(yaw1) && finite_d(v_avg), "minsnap_solve: yaw0, yaw1 and v_avg must be finite");
    double o[3] = {0.0, 0.0, 0.0};
    if (cells) {
        MNF_REQUIRE(origin_host, "minsnap_solve: origin_host is null");
        MNF_REQUIRE(resolution > 0.0 && resolution <= 1.79e308, "minsnap_solve: resolution must be positive and finite (got %g)", resolution);
        MNF_REQUIRE(finite_d(height), "minsnap_solve: height is not finite");
        for (int k = 0; k < 3; ++k) {
            MNF_REQUIRE(finite_d(origin_host[k]), "minsnap_solve: origin_host[%d] is not finite", k);
            o[k] = origin_host[k];
        }
    }
    MNF_REQUIRE(aligned8(points) && aligned8(offsets) && aligned8(coeffs) && aligned8(delta_t) && aligned8(t_keyframes) && aligned8(yaw_execute) && aligned8(workspace),
                "minsnap_solve: float64 and int64 arrays and the workspace must be 8-byte aligned");
    if (n_traj == 0) return MNF_OK;
    MNF_REQUIRE(offsets && n_segments && status, "minsnap_solve: a null pointer");
    MNF_REQUIRE((coeffs && delta_t && t_keyframes && yaw_execute) || n_waypoints == 0, "minsnap_solve: a null output");
    MNF_REQUIRE(workspace && workspace_bytes >= mnf_minsnap_workspace_bytes(n_traj, n_waypoints, 0), "minsnap_solve: the workspace holds %lld bytes, %lld are needed",
                (long long)workspace_bytes, (long long)mnf_minsnap_workspace_bytes(n_traj, n_waypoints, 0));
    hipStream_t s = as_stream(stream);
    ProfScope prof("minsnap_solve", s);
    double *ws = static_cast<double *>(workspace);
    hipLaunchKernelGGL(solve_kernel, dim3((unsigned)n_traj), dim3(64), 0, s, points, cells, offsets, n_waypoints, resolution, o[0], o[1], o[2], height, yaw0, yaw1,
                       v_avg, coeffs, delta_t, t_keyframes, yaw_execute, n_segments, status, ws, ws + n_waypoints);
    return launch_status("solve_kernel");
}

extern "C" int mnf_minsnap_sample_count(const double *delta_t, const int64_t *offsets, int64_t n_waypoints, const int32_t *n_segments, const int32_t *status,
                                        int64_t n_traj, double rate, int64_t min_samples, int64_t max_samples, int64_t *counts, int32_t *sample_status,
                                        void *workspace, int64_t workspace_bytes, mnf_stream_t stream) {
    MNF_REQUIRE(n_traj >= 0 && n_traj < ((int64_t)1 << 31), "minsnap_sample_count: n_traj outside [0, 2^31) (%lld)", (long long)n_traj);
    MNF_REQUIRE(n_waypoints >= 0 && n_waypoints < ((int64_t)1 << 31), "minsnap_sample_count: n_waypoints outside [0, 2^31) (%lld)", (long long)n_waypoints);
    MNF_REQUIRE(rate > 0.0 && rate <= 1.79e308, "minsnap_sample_count: rate must be positive and finite (got %g)", rate);
    MNF_REQUIRE(min_samples >= 1 && min_samples < ((int64_t)1 << 31), "minsnap_sample_count: min_samples outside [1, 2^31) (%lld)", (long long)min_samples);
    MNF_REQUIRE(max_samples >= 1 && max_samples < ((int64_t)1 << 31), "minsnap_sample_count: max_samples outside [1, 2^31) (%lld)", (long long)max_samples);
    MNF_REQUIRE(aligned8(delta_t) && aligned8(offsets) && aligned8(counts) && aligned8(workspace),
                "minsnap_sample_count: float64 and int64 arrays and the workspace must be 8-byte aligned");
    if (n_traj == 0) return MNF_OK;
    MNF_REQUIRE(offsets && n_segments && status && counts && sample_status, "minsnap_sample_count: a null pointer");
    MNF_REQUIRE(delta_t || n_waypoints == 0, "minsnap_sample_count: delta_t is null");
    MNF_REQUIRE(workspace && workspace_bytes >= n_traj * max_samples * 8, "minsnap_sample_count: the workspace holds %lld bytes, %lld are needed",
                (long long)workspace_bytes, (long long)(n_traj * max_samples * 8));
    hipStream_t s = as_stream(stream);
    ProfScope prof("minsnap_sample_count", s);
    hipLaunchKernelGGL(sample_count_kernel, dim3(blocks_for(n_traj, 64)), dim3(64), 0, s, delta_t, offsets, n_waypoints, n_segments, status, n_traj, rate,
                       (long long)min_samples, (long long)max_samples, reinterpret_cast<long long *>(counts), sample_status, static_cast<double *>(workspace));
    return launch_status("sample_count_kernel");
}

extern "C" int mnf_minsnap_sample_fill(const double *coeffs, const double *delta_t, const double *t_keyframes, const int64_t *offsets, int64_t n_waypoints,
                                       const int32_t *n_segments, int64_t n_traj, int64_t max_samples, const int64_t *sample_offsets, int64_t n_samples,
                                       const int64_t *pose_offsets, int64_t n_poses, const double *look_quats, int32_t n_look, double *flat_x, double *times,
                                       double *derivatives, double *yaw, double *poses, const void *workspace, int64_t workspace_bytes, mnf_stream_t stream) {
    MNF_REQUIRE(n_traj >= 0 && n_traj < ((int64_t)1 << 31), "minsnap_sample_fill: n_traj outside [0, 2^31) (%lld)", (long long)n_traj);
    MNF_REQUIRE(n_waypoints >= 0 && n_waypoints < ((int64_t)1 << 31), "minsnap_sample_fill: n_waypoints outside [0, 2^31) (%lld)", (long long)n_waypoints);
    MNF_REQUIRE(max_samples >= 1 && max_samples < ((int64_t)1 << 31), "minsnap_sample_fill: max_samples outside [1, 2^31) (%lld)", (long long)max_samples);
    MNF_REQUIRE(n_samples >= 0 && n_samples < ((int64_t)1 << 40), "minsnap_sample_fill: n_samples outside [0, 2^40) (%lld)", (long long)n_samples);
    MNF_REQUIRE(n_poses >= 0 && n_poses < ((int64_t)1 << 40), "minsnap_sample_fill: n_poses outside [0, 2^40) (%lld)", (long long)n_poses);
    MNF_REQUIRE(n_look >= 0, "minsnap_sample_fill: n_look is negative (%d)", n_look);
    MNF_REQUIRE(aligned8(coeffs) && aligned8(delta_t) && aligned8(t_keyframes) && aligned8(offsets) && aligned8(sample_offsets) && aligned8(pose_offsets) &&
                    aligned8(look_quats) && aligned8(flat_x) && aligned8(times) && aligned8(derivatives) && aligned8(yaw) && aligned8(poses) && aligned8(workspace),
                "minsnap_sample_fill: float64 and int64 arrays and the workspace must be 8-byte aligned");
    if (n_traj == 0 || n_poses == 0) return MNF_OK;
    MNF_REQUIRE(coeffs && delta_t && t_keyframes && offsets && n_segments && sample_offsets && pose_offsets && poses, "minsnap_sample_fill: a null pointer");
    MNF_REQUIRE((flat_x && times) || n_samples == 0, "minsnap_sample_fill: flat_x or times is null");
    MNF_REQUIRE(look_quats || n_look == 0, "minsnap_sample_fill: look_quats is null");
    MNF_REQUIRE(workspace && workspace_bytes >= n_traj * max_samples * 8, "minsnap_sample_fill: the workspace holds %lld bytes, %lld are needed",
                (long long)workspace_bytes, (long long)(n_traj * max_samples * 8));
    hipStream_t s = as_stream(stream);
    ProfScope prof("minsnap_sample_fill", s);
    hipLaunchKernelGGL(sample_fill_kernel, dim3(blocks_for(n_poses)), dim3(256), 0, s, coeffs, delta_t, t_keyframes, offsets, n_waypoints, n_segments, n_traj,
                       max_samples, sample_offsets, n_samples, pose_offsets, n_poses, look_quats, (int)n_look, flat_x, times, derivatives, yaw, poses,
                       static_cast<const double *>(workspace));
    return launch_status("sample_fill_kernel");
}
