"""numpy restatement of the min-snap trajectory unit (csrc/minsnap.hip, include/mi355nerf.h "min-snap candidate trajectories"): the
reference's time allocation in its order of operations, its square system A c = b in the row order that makes it banded, solved with
scipy.linalg.solve_banded, the sample times as sample_traj's loop forms them, MinSnap.update's evaluation, update_ref's attitude and
sample_traj's axis shuffle in closed form.  `dense=True` solves as the reference does (four SVD rank tests and four dense solves of the
system in its own row order): the timing yardstick of tools/minsnap_time.py."""
import math
import os

import numpy as np

OK, NULL, REJECTED_SHORT, SINGULAR, TOO_LONG, NOT_FINITE = 0, 1, 2, 4, 8, 16
SAMPLE_OVERFLOW, SAMPLE_INVALID = 32, 64
MAX_SEGMENTS = 1023
G = 9.81
EPS = np.finfo(np.float64).eps
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "minsnap_trajectories.npz")


def waypoints_of_cells(cells, resolution, origin, height=1.7):
    """trace_paths lists the goal first: reversed, index * resolution + aabb[:3] as sample_traj forms dij_waypoints."""
    c = np.asarray(cells, np.int64).reshape(-1, 2)[::-1]
    o = np.asarray(origin, np.float64)
    out = np.empty((c.shape[0], 3), np.float64)
    out[:, 0] = c[:, 0].astype(np.float64) * resolution + o[0]
    out[:, 1] = c[:, 1].astype(np.float64) * resolution + o[1]
    out[:, 2] = height + o[2]
    return out


def time_allocation(points, v_avg=0.5):
    """-> (kept points [m+1,3], seg_dist over ALL waypoints, delta_t [m], t_keyframes [m+1]); m = 0: one waypoint is left."""
    points = np.asarray(points, np.float64).reshape(-1, 3)
    d = np.diff(points, axis=0)
    seg_dist = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    kept = points[np.append(True, seg_dist > 1e-2)]
    m = kept.shape[0] - 1
    delta_t = np.zeros(m)
    vi, cum = 0.0, 0.0
    total = float(np.sum(seg_dist)) if seg_dist.size else 0.0
    for i in range(m):
        cum += float(seg_dist[i])
        vf = min(min(cum, v_avg), total - cum)
        delta_t[i] = float(seg_dist[i]) * 2 / (vf + vi + 1e-4)
        vi = vf
    t_keyframes = np.concatenate(([0.0], np.cumsum(delta_t)))
    return kept, seg_dist, delta_t, t_keyframes


def yaw_execute(t_keyframes, yaw0, yaw1):
    return t_keyframes / (t_keyframes[-1] + 1e-4) * (yaw1 - yaw0) + yaw0


def _falling(k, d):
    f = 1.0
    for q in range(d):
        f *= k - q
    return f


def banded_rows(delta_t):
    """The rows of A in the banded order: a list of (row, {column: value})."""
    m = len(delta_t)
    rows = [{1: 1.0}, {2: 2.0}, {3: 6.0}]
    for i in range(m):
        dt = float(delta_t[i])
        rows.append({8 * i: 1.0})
        rows.append({8 * i + k: dt ** k for k in range(8)})
        for d in (1, 2, 3) if i == m - 1 else (1, 2, 3, 4, 5, 6):
            row = {8 * i + k: _falling(k, d) * dt ** (k - d) for k in range(d, 8)}
            if i < m - 1:
                row = {c: -v for c, v in row.items()}
                row[8 * i + 8 + d] = _falling(d, d)
            rows.append(row)
    assert len(rows) == 8 * m
    return rows


def dense_banded_order(delta_t):
    n = 8 * len(delta_t)
    A = np.zeros((n, n))
    for r, row in enumerate(banded_rows(delta_t)):
        for c, v in row.items():
            A[r, c] = v
    return A


def band_storage(delta_t):
    """scipy.linalg.solve_banded's ab for (l, u) = (4, 4): ab[4 + r - c, c] = A[r, c]."""
    n = 8 * len(delta_t)
    ab = np.zeros((9, n))
    for r, row in enumerate(banded_rows(delta_t)):
        for c, v in row.items():
            assert -4 <= r - c <= 4, (r, c)
            ab[4 + r - c, c] = v
    return ab


def rhs_banded_order(keyframes):
    """keyframes [m+1, axes] -> b [8 m, axes]."""
    keyframes = np.asarray(keyframes, np.float64)
    m = keyframes.shape[0] - 1
    b = np.zeros((8 * m, keyframes.shape[1]))
    for i in range(m):
        b[3 + 8 * i] = keyframes[i]
        b[4 + 8 * i] = keyframes[i + 1]
    return b


def _reference_system(keyframes, delta_t):
    """get_1d_equality_constraints in its own row order (one axis)."""
    m = len(delta_t)
    rows = banded_rows(delta_t)
    order = [None] * (8 * m)
    order[8 * m - 6], order[8 * m - 4], order[8 * m - 2] = 0, 1, 2
    for i in range(m):
        order[i] = 3 + 8 * i
        order[m + i] = 4 + 8 * i
        if i < m - 1:
            for d in range(6):
                order[2 * m + 6 * i + d] = 5 + 8 * i + d
    order[8 * m - 5], order[8 * m - 3], order[8 * m - 1] = 8 * m - 3, 8 * m - 2, 8 * m - 1
    A = np.zeros((8 * m, 8 * m))
    b_band = rhs_banded_order(np.asarray(keyframes, np.float64).reshape(-1, 1))[:, 0]
    b = np.zeros(8 * m)
    for r, src in enumerate(order):
        for c, v in rows[src].items():
            A[r, c] = v
        b[r] = b_band[src]
    return A, b


def solve(delta_t, keyframes, dense=False):
    """keyframes [m+1,4] (x, y, z, yaw_execute) -> c [m,4,8], lowest power first; None where the dense route's rank test refuses."""
    m = len(delta_t)
    keyframes = np.asarray(keyframes, np.float64)
    if dense:
        cols = []
        systems = [_reference_system(keyframes[:, a], delta_t) for a in range(4)]
        if not all(np.linalg.matrix_rank(A) == A.shape[0] for A, _ in systems):
            return None
        for A, b in systems:
            cols.append(np.linalg.solve(A, b))
        x = np.stack(cols, axis=1)
    else:
        from scipy.linalg import solve_banded
        x = solve_banded((4, 4), band_storage(delta_t), rhs_banded_order(keyframes))
    return np.ascontiguousarray(x.reshape(m, 8, 4).transpose(0, 2, 1))


def residual_bound(delta_t, keyframes, coeffs):
    """(|A c - b|_inf, 64 eps (|A|_inf |c|_inf + |b|_inf)) over the four axes, A assembled here from delta_t (row by row: any m)."""
    m = len(delta_t)
    b = rhs_banded_order(keyframes)
    c = np.asarray(coeffs, np.float64).reshape(m, 4, 8).transpose(0, 2, 1).reshape(8 * m, 4)
    res, norm = 0.0, 0.0
    for r, row in enumerate(banded_rows(delta_t)):
        cols = np.fromiter(row.keys(), np.int64, len(row))
        vals = np.fromiter(row.values(), np.float64, len(row))
        res = max(res, float(np.abs(vals @ c[cols] - b[r]).max()))
        norm = max(norm, float(np.abs(vals).sum()))
    bound = 64 * EPS * (norm * np.abs(c).max() + np.abs(b).max())
    return res, float(bound)


def sample_times(delta_t, rate=20, min_samples=20):
    t_final = np.sum(delta_t)
    n = max(int(t_final * rate), min_samples)
    t_step = t_final / n
    time = [0]
    while not time[-1] >= t_final:
        time.append(time[-1] + t_step)
    return np.array(time, dtype=float)


def _polyval(c, order, tau):
    """c [..., 8] lowest power first; np.polyval of np.polyder(flip(c), order) at tau."""
    y = None
    for k in range(7, order - 1, -1):
        pv = c[..., k]
        for q in range(order):
            pv = pv * float(k - q)
        y = pv if y is None else y * tau + pv
    return y


def evaluate(coeffs, delta_t, t_keyframes, times):
    """MinSnap.update at every time -> dict of x, x_dot, x_ddot, x_dddot, x_ddddot [S,3], yaw, yaw_dot, yaw_ddot [S]."""
    m = len(delta_t)
    t = np.clip(np.asarray(times, np.float64), t_keyframes[0], t_keyframes[-1])
    seg = np.minimum(np.searchsorted(t_keyframes[:-1] + delta_t, t, side="left"), m - 1)
    tau = t - t_keyframes[seg]
    c = np.asarray(coeffs, np.float64)[seg]                                           # [S,4,8]
    out = {}
    for order, name in enumerate(("x", "x_dot", "x_ddot", "x_dddot", "x_ddddot")):
        out[name] = np.stack([_polyval(c[:, a], order, tau) for a in range(3)], axis=1)
    for order, name in enumerate(("yaw", "yaw_dot", "yaw_ddot")):
        out[name] = _polyval(c[:, 3], order, tau)
    return out


def attitude(x_ddot, yaw):
    """-> (cmd_q as update_ref returns it, the quaternion after sample_traj's axis shuffle), both [S,4] (x, y, z, w)."""
    a = np.asarray(x_ddot, np.float64)
    tx, ty, tz = a[:, 0] + 0.0, a[:, 1] + 0.0, a[:, 2] + G
    tn = np.sqrt((tx * tx + ty * ty) + tz * tz)
    b3 = np.stack([tx / tn, ty / tn, tz / tn], axis=1)
    c1 = np.stack([np.cos(yaw), np.sin(yaw), np.zeros_like(yaw)], axis=1)
    b2 = np.cross(b3, c1)
    b2 = b2 / np.sqrt((b2[:, 0] * b2[:, 0] + b2[:, 1] * b2[:, 1]) + b2[:, 2] * b2[:, 2])[:, None]
    b1 = np.cross(b2, b3)
    R = np.stack([b1, b2, b3], axis=2)                                                # R[s, r, c]: column c is b_{c+1}
    q = np.empty((a.shape[0], 4))
    for s in range(a.shape[0]):
        M = R[s]
        trace = (M[0, 0] + M[1, 1]) + M[2, 2]
        dec = [M[0, 0], M[1, 1], M[2, 2], trace]
        choice = 0
        for k in range(1, 4):
            if dec[k] > dec[choice]:
                choice = k
        u = np.empty(4)
        if choice != 3:
            i = choice
            j = (i + 1) % 3
            k = (j + 1) % 3
            u[i] = 1.0 - trace + 2.0 * M[i, i]
            u[j] = M[j, i] + M[i, j]
            u[k] = M[k, i] + M[i, k]
            u[3] = M[k, j] - M[j, k]
        else:
            u[0] = M[2, 1] - M[1, 2]
            u[1] = M[0, 2] - M[2, 0]
            u[2] = M[1, 0] - M[0, 1]
            u[3] = 1.0 + trace
        q[s] = u / math.sqrt(((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2]) + u[3] * u[3])
    sign = np.where(q[:, 3] < 0.0, -1.0, 1.0)
    shuffled = np.stack([-(sign * q[:, 0]), sign * q[:, 2], -(sign * q[:, 1]), sign * q[:, 3]], axis=1)
    return q, shuffled


def look_quats(angles=None):
    """R.from_euler("y", ang, degrees=True).as_quat() for every angle, signs as scipy leaves them."""
    angles = np.linspace(0, 360, 20) if angles is None else np.asarray(angles, np.float64)
    return np.array([[0.0, math.sin(a / 2), 0.0, math.cos(a / 2)] for a in np.deg2rad(angles)]).reshape(-1, 4)


def quat_matrix(q):
    """Rotation matrices of unit quaternions (x, y, z, w) [S,4] -> [S,3,3]."""
    q = np.asarray(q, np.float64)
    q = q / np.linalg.norm(q, axis=1, keepdims=True)
    x, y, z, w = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], axis=1),
                     np.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], axis=1),
                     np.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], axis=1)], axis=1)


def restate(points, yaw=(2 * math.pi, 0.0), v_avg=0.5, rate=20, min_samples=20, look_angles=None, dense=False):
    """One path, the way sample_traj treats it -> a dict with `status` and, for an accepted path, everything the golden stores."""
    points = np.asarray(points, np.float64).reshape(-1, 3)
    if not np.isfinite(points).all():
        return {"status": NOT_FINITE, "m": 0}
    kept, seg_dist, delta_t, tk = time_allocation(points, v_avg)
    m = kept.shape[0] - 1
    if m == 0:
        return {"status": NULL, "m": 0}
    if m == 1:
        return {"status": REJECTED_SHORT, "m": 1}
    if m > MAX_SEGMENTS:
        return {"status": TOO_LONG, "m": m}
    if not (np.isfinite(delta_t).all() and (delta_t > 0).all()):
        return {"status": SINGULAR, "m": m}                                           # a repeated waypoint inside the path: the reference's delta_t is 0
    ye = yaw_execute(tk, yaw[0], yaw[1])
    keyframes = np.concatenate([kept, ye[:, None]], axis=1)
    coeffs = solve(delta_t, keyframes, dense=dense)
    if coeffs is None:
        return {"status": SINGULAR, "m": m}
    times = sample_times(delta_t, rate, min_samples)
    flat = evaluate(coeffs, delta_t, tk, times)
    cmd_q, quat = attitude(flat["x_ddot"], flat["yaw"])
    xzy = flat["x"][:, [0, 2, 1]]
    look = look_quats(look_angles)
    poses = np.concatenate([np.concatenate([xzy, quat], axis=1),
                            np.concatenate([np.repeat(xzy[-1:], look.shape[0], axis=0), look], axis=1)], axis=0)
    return {"status": OK, "m": m, "points": kept, "delta_t": delta_t, "t_keyframes": tk, "yaw_execute": ye, "keyframes": keyframes, "coeffs": coeffs,
            "times": times, "flat": flat, "cmd_q": cmd_q, "poses": poses}


# ---------------------------------------------------------------------------------------------------------------- the golden fixture
QUANTITIES = ("coeffs", "x", "x_ddot", "yaw", "pose_position", "pose_rotation")


def golden_paths(g):
    """The fixture (tests/golden/minsnap_trajectories.npz) as a list of dicts, one per path; `cells` goal first, as a trace lists them."""
    out = []
    for p in range(int(g["n_paths"])):
        d = {"name": str(g["names"][p]), "cells": g["cells"][g["cell_offsets"][p]:g["cell_offsets"][p + 1]], "accepted": bool(g["accepted"][p]),
             "null": bool(g["null"][p]), "initialized": bool(g["initialized"][p]), "m": int(g["m"][p])}
        if d["accepted"]:
            s0, s1 = g["seg_offsets"][p], g["seg_offsets"][p + 1]
            k0, k1 = g["key_offsets"][p], g["key_offsets"][p + 1]
            a0, a1 = g["sample_offsets"][p], g["sample_offsets"][p + 1]
            q0, q1 = g["pose_offsets"][p], g["pose_offsets"][p + 1]
            d.update(delta_t=g["delta_t"][s0:s1], coeffs=g["c_opt"][s0:s1], t_keyframes=g["t_keyframes"][k0:k1], yaw_execute=g["yaw_execute"][k0:k1],
                     times=g["times"][a0:a1], x=g["x"][a0:a1], x_ddot=g["x_ddot"][a0:a1], yaw=g["yaw"][a0:a1], cmd_q=g["cmd_q"][a0:a1],
                     poses=g["poses"][q0:q1], cond=float(g["cond"][p]), N=int(g["N"][p]))
        out.append(d)
    return out


def expected_status(path):
    return OK if path["accepted"] else NULL if path["null"] else REJECTED_SHORT if path["m"] == 1 else SINGULAR


def deviations(got, want):
    """Largest deviation per quantity of a restated (or device) path `got` from a golden path `want`.  got: coeffs, x, x_ddot, yaw, poses."""
    n_look = want["poses"].shape[0] - want["times"].shape[0]
    S = want["times"].shape[0]
    Rg, Rw = quat_matrix(got["poses"][:S, 3:]), quat_matrix(want["poses"][:S, 3:])
    return {"coeffs": float(np.abs(got["coeffs"] - want["coeffs"]).max()), "x": float(np.abs(got["x"] - want["x"]).max()),
            "x_ddot": float(np.abs(got["x_ddot"] - want["x_ddot"]).max()), "yaw": float(np.abs(got["yaw"] - want["yaw"]).max()),
            "pose_position": float(np.abs(got["poses"][:, :3] - want["poses"][:, :3]).max()), "pose_rotation": float(np.abs(Rg - Rw).max()),
            "n_look": n_look}


def forward_bounds(p):
    """The forward bounds that follow from the residual criterion, for one golden path (tests/test_minsnap_cpu.py derives them) -> dict per
    quantity, with the reference's own residual, rho and the keyframes [m+1,4]."""
    A = dense_banded_order(p["delta_t"])
    ainv = np.abs(np.linalg.inv(A)).sum(axis=1).max()
    keyframes = np.concatenate([p_points(p), p["yaw_execute"][:, None]], axis=1)
    res_ref, rho_ref = residual_bound(p["delta_t"], keyframes, p["coeffs"])
    tau = float(p["delta_t"].max())
    dc = ainv * (rho_ref + max(rho_ref, res_ref))
    dx = dc * sum(tau ** k for k in range(8))
    da = dc * sum(k * (k - 1) * tau ** (k - 2) for k in range(2, 8))
    amax = float(np.abs(p["x_ddot"]).max())
    return {"coeffs": dc, "x": dx, "x_ddot": da, "yaw": dx, "pose_position": dx, "pose_rotation": 4 * (da / (G - amax) + dx) + 64 * EPS,
            "residual_reference": res_ref, "rho": rho_ref, "keyframes": keyframes}


def p_points(p):
    """The kept waypoints of a golden path: the reference's own polynomials at the keyframes would do, the cells do it exactly."""
    g = np.load(GOLDEN)
    pts = waypoints_of_cells(p["cells"], float(g["resolution"]), g["origin"], float(g["height"]))
    return time_allocation(pts)[0]


def write_parity(section, lines):
    """profiles/minsnap_parity.txt holds one block of lines per section ("restatement": this file against the reference, written by the CPU
    test; "device": the library against the reference, written by the GPU test); a section's lines all start with its name."""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "minsnap_parity.txt")
    head = ["# largest deviation per quantity from the reference's answers (tests/golden/minsnap_trajectories.npz), per path and over all paths;",
            "# written by tests/test_minsnap_cpu.py (restatement) and tests/test_gpu_minsnap.py (device, allowed 8 x the restatement's worst)"]
    old = []
    if os.path.exists(path):
        old = [ln.rstrip("\n") for ln in open(path) if not ln.startswith("#") and not ln.startswith(section) and ln.strip()]
    body = (list(lines) + old) if section == "restatement" else (old + list(lines))
    with open(path, "w") as f:
        f.write("\n".join(head + body) + "\n")
