"""Min-snap candidate trajectories on the device (csrc/minsnap.hip): the inner block of sample_traj (planning/planning_funcs.py:328-397),
which turns every traced path into a `MinSnap` curve (planning/rotorpy/rotorpy/trajectories/minsnap.py), samples it 20 times a second, asks
`SE3Control.update_ref` for cmd_q per sample, shuffles the quaternion's axes and appends 20 look-around poses.  Here the chain
`draw_goals` -> `trace_paths` -> curves -> samples -> `ClearanceField.trajectory_clearance` -> poses stays on the device; the definition
(the band, the order of operations, the statuses) is in include/mi355nerf.h ("min-snap candidate trajectories") and DESIGN.md.

A curve is accepted by three rules that stand in for the reference's SVD rank test: one waypoint left is `NULL`, two are
`REJECTED_SHORT` (the reference always refuses them), and from two segments on the curve is accepted unless a pivot of the elimination falls
below n eps |A|_inf (`SINGULAR`, this project's own criterion)."""
import ctypes
import math

import numpy as np
import torch

from . import _lib as L
from .planning import trace_paths

OK, NULL, REJECTED_SHORT, SINGULAR, TOO_LONG, NOT_FINITE = 0, 1, 2, 4, 8, 16
SAMPLE_OVERFLOW, SAMPLE_INVALID = 32, 64
MAX_SEGMENTS = 1023
DEFAULT_MAX_SAMPLES = 16384
DEFAULT_YAW = (2 * math.pi, 0.0)               # sample_traj's np.linspace(2 * np.pi, 0, n) enters MinSnap by its two ends


def look_quaternions(angles_deg):
    """[n,4] float64 (x, y, z, w): `R.from_euler("y", a, degrees=True).as_quat()` per angle, (0, sin(a/2), 0, cos(a/2)) with the signs scipy
    leaves (w = -1 at 360 degrees).  math.sin / math.cos: the C library's, which scipy calls too."""
    a = np.deg2rad(np.asarray(angles_deg, np.float64).reshape(-1))
    return np.array([[0.0, math.sin(v / 2), 0.0, math.cos(v / 2)] for v in a], np.float64).reshape(-1, 4)


def _offsets(offsets, n, device):
    if offsets is None:
        return torch.tensor([0, n], dtype=torch.int64, device=device)
    off = offsets if torch.is_tensor(offsets) else torch.from_numpy(np.ascontiguousarray(np.asarray(offsets, np.int64)))
    off = L.contig(off.to(device), torch.int64).reshape(-1)
    if int(off.shape[0]) < 1:
        raise ValueError("offsets is [T+1]")
    return off


class MinSnapCurves:
    """Device tensors.  `coeffs` float64 [W,4,8] (segment row, axis x / y / z / yaw, power, lowest first), `delta_t`, `t_keyframes`,
    `yaw_execute` float64 [W], all packed at `seg_offsets` int64 [T+1], which are the waypoint offsets the curves were solved from: trajectory
    t has `n_segments[t]` segment rows from seg_offsets[t] on and one keyframe more.  `status` int32 [T] (OK, NULL, REJECTED_SHORT, SINGULAR,
    TOO_LONG, NOT_FINITE).  Rows of refused trajectories are zero."""

    def __init__(self, coeffs, delta_t, t_keyframes, yaw_execute, seg_offsets, n_segments, status):
        self.coeffs, self.delta_t, self.t_keyframes, self.yaw_execute = coeffs, delta_t, t_keyframes, yaw_execute
        self.seg_offsets, self.n_segments, self.status = seg_offsets, n_segments, status
        self.device = status.device

    def __len__(self):
        return int(self.status.shape[0])

    @torch.no_grad()
    def sample(self, rate=20, min_samples=20, look_angles=None, derivatives=False, max_samples=None, host=False):
        """sample_traj's sampling loop and pose rows for every accepted curve.  -> dict of device tensors:
          "counts" int64 [T] (0 for a refused curve), "sample_status" int32 [T] (SAMPLE_OVERFLOW: more than `max_samples` samples, count 0),
          "sample_offsets" int64 [T+1], "flat_x" float64 [S,3] = flat["x"] (what `trajectory_clearance(planner_axes=True)` takes), "times" [S],
          "pose_offsets" int64 [T+1], "poses" float64 [P,7]: per sample the x, z, y position and the shuffled cmd_q, then one row per look
          angle (degrees, default np.linspace(0, 360, 20)) at the last sample's position;
          derivatives=True adds "derivatives" [S,12] (x_dot, x_ddot, x_dddot, x_ddddot) and "yaw" [S,3] (yaw, yaw_dot, yaw_ddot).
        The two totals are the one host read.  host=True adds "trajectories": the list of [len,7] float64 arrays sample_traj returns, refused
        curves left out, with "kept" and "refused": their indices."""
        lib = L.load_library()
        dev = self.device
        T = len(self)
        W = int(self.delta_t.shape[0])
        max_samples = DEFAULT_MAX_SAMPLES if max_samples is None else int(max_samples)
        look = look_quaternions(np.linspace(0, 360, 20) if look_angles is None else look_angles)
        n_look = int(look.shape[0])
        look_dev = torch.from_numpy(look).to(dev) if n_look else None
        counts = torch.zeros(T, dtype=torch.int64, device=dev)
        sstat = torch.zeros(T, dtype=torch.int32, device=dev)
        need = int(lib.mnf_minsnap_workspace_bytes(T, 0, max_samples))
        if need < 0:
            raise L.MnfError(f"{T} trajectories of up to {max_samples} samples are outside what the sample workspace holds")
        ws = torch.empty(need // 8 + 1, dtype=torch.float64, device=dev)
        if T:
            L.launch(lib.mnf_minsnap_sample_count, L.ptr(self.delta_t), L.ptr(self.seg_offsets), W, L.ptr(self.n_segments), L.ptr(self.status), T, float(rate),
                     int(min_samples), max_samples, L.ptr(counts), L.ptr(sstat), L.ptr(ws), need)
        soff = torch.zeros(T + 1, dtype=torch.int64, device=dev)
        poff = torch.zeros(T + 1, dtype=torch.int64, device=dev)
        if T:
            soff[1:] = torch.cumsum(counts, 0)
            poff[1:] = torch.cumsum(torch.where(counts > 0, counts + n_look, torch.zeros_like(counts)), 0)
        S, P = (int(v) for v in torch.stack([soff[-1], poff[-1]]).cpu().tolist())
        flat_x = torch.zeros(max(S, 1), 3, dtype=torch.float64, device=dev)
        times = torch.zeros(max(S, 1), dtype=torch.float64, device=dev)
        poses = torch.zeros(max(P, 1), 7, dtype=torch.float64, device=dev)
        der = torch.zeros(max(S, 1), 12, dtype=torch.float64, device=dev) if derivatives else None
        yaw = torch.zeros(max(S, 1), 3, dtype=torch.float64, device=dev) if derivatives else None
        if T and P:
            L.launch(lib.mnf_minsnap_sample_fill, L.ptr(self.coeffs), L.ptr(self.delta_t), L.ptr(self.t_keyframes), L.ptr(self.seg_offsets), W,
                     L.ptr(self.n_segments), T, max_samples, L.ptr(soff), S, L.ptr(poff), P, L.ptr(look_dev), n_look, L.ptr(flat_x), L.ptr(times), L.ptr(der),
                     L.ptr(yaw), L.ptr(poses), L.ptr(ws), need)
        out = {"counts": counts, "sample_status": sstat, "sample_offsets": soff, "flat_x": flat_x[:S], "times": times[:S], "pose_offsets": poff,
               "poses": poses[:P]}
        if derivatives:
            out["derivatives"], out["yaw"] = der[:S], yaw[:S]
        if host:
            p, o = poses[:P].cpu().numpy(), poff.cpu().numpy()
            kept = [t for t in range(T) if o[t + 1] > o[t]]
            out["trajectories"] = [p[o[t]:o[t + 1]].copy() for t in kept]
            out["kept"], out["refused"] = kept, [t for t in range(T) if o[t + 1] == o[t]]
        return out


@torch.no_grad()
def _solve(points, cells, offsets, resolution, origin, height, yaw, v_avg, device):
    lib = L.load_library()
    src = points if points is not None else cells
    L.require_gpu(src)
    W = int(src.shape[0])
    off = _offsets(offsets, W, device)
    T = int(off.shape[0]) - 1
    need = int(lib.mnf_minsnap_workspace_bytes(T, W, 0))
    if need < 0:
        raise L.MnfError(f"{T} trajectories of {W} waypoints are outside what the solve takes")
    rows = max(W, 1)
    coeffs = torch.zeros(rows, 4, 8, dtype=torch.float64, device=device)
    delta_t = torch.zeros(rows, dtype=torch.float64, device=device)
    tk = torch.zeros(rows, dtype=torch.float64, device=device)
    ye = torch.zeros(rows, dtype=torch.float64, device=device)
    nseg = torch.zeros(T, dtype=torch.int32, device=device)
    status = torch.full((T,), NULL, dtype=torch.int32, device=device)
    ws = torch.empty(need // 8 + 1, dtype=torch.float64, device=device)
    o = (ctypes.c_double * 3)(*[float(v) for v in (origin if origin is not None else (0.0, 0.0, 0.0))])
    if T:
        L.launch(lib.mnf_minsnap_solve, L.ptr(points) if points is not None and W else None, L.ptr(cells) if cells is not None and W else None, L.ptr(off), T, W,
                 float(resolution), o, float(height), float(yaw[0]), float(yaw[1]), float(v_avg), L.ptr(coeffs), L.ptr(delta_t), L.ptr(tk), L.ptr(ye), L.ptr(nseg),
                 L.ptr(status), L.ptr(ws), need, device=device)
    return MinSnapCurves(coeffs[:W], delta_t[:W], tk[:W], ye[:W], off, nseg, status)


def min_snap(points, offsets=None, yaw=DEFAULT_YAW, v_avg=0.5, device="cuda:0"):
    """`MinSnap(points[t], yaw_angles=np.linspace(yaw[0], yaw[1], n), v_avg).initialize()` for every trajectory of `points` [W,3] float64
    (device or host) packed at `offsets` [T+1] (None: one trajectory) -> `MinSnapCurves`.  One launch, no host copy."""
    p = points if torch.is_tensor(points) else torch.from_numpy(np.ascontiguousarray(np.asarray(points, np.float64)))
    device = p.device if p.is_cuda else torch.device(device)
    p = L.contig(p.to(device), torch.float64).reshape(-1, 3)
    return _solve(p, None, offsets, 1.0, None, 0.0, yaw, v_avg, device)


def min_snap_cells(cells, offsets, resolution, origin, height=1.7, yaw=DEFAULT_YAW, v_avg=0.5, device="cuda:0"):
    """The curves of `trace_paths` output as it stands: `cells` int32 [W,2], goal first, packed at `offsets`.  Every path is reversed and
    becomes (cx * resolution + origin[0], cy * resolution + origin[1], height + origin[2]), sample_traj's dij_waypoints; `origin` = aabb[:3]."""
    c = cells if torch.is_tensor(cells) else torch.from_numpy(np.ascontiguousarray(np.asarray(cells, np.int32)))
    device = c.device if c.is_cuda else torch.device(device)
    c = L.contig(c.to(device), torch.int32).reshape(-1, 2)
    origin = [float(v) for v in (origin.detach().cpu().reshape(-1)[:3].tolist() if torch.is_tensor(origin) else np.asarray(origin, np.float64).reshape(-1)[:3])]
    return _solve(None, c, offsets, resolution, origin, height, yaw, v_avg, device)


@torch.no_grad()
def candidate_trajectories(dijkstra, start_xy, goals_xy, aabb, height=1.7, yaw=DEFAULT_YAW, v_avg=0.5, rate=20, min_samples=20, look_angles=None,
                           max_samples=None, clearance=None, radius=0.0, host=False):
    """sample_traj's candidates for one start and many goals: `dijkstra.planning_many`'s trace (`goals_xy` in the planner's metres, as
    `planning` takes them), `min_snap_cells` on the traced cells and `MinSnapCurves.sample`, with the paths and the curves never on the host.
    -> the dict of `sample` plus "curves", "paths", "path_offsets", "trace_info"; a goal that is not reached has no path and status NULL.
    `clearance=field, radius=r` runs `field.trajectory_clearance(flat_x, sample_offsets, planner_axes=True, radius=r)` in the same call and
    adds its dict as "clearance" and "certified" bool [T]: the field's verdict, and False for a curve without samples."""
    goals_xy = list(goals_xy)
    dev = dijkstra.device
    field = dijkstra._field(start_xy[0], start_xy[1])
    if field is None:
        raise L.MnfError("the start lies outside the planner's map")
    big = 1 << 30
    cells = [(0, max(-1, min(int(dijkstra.calc_xy_index(gx, dijkstra.min_x)), big)), max(-1, min(int(dijkstra.calc_xy_index(gy, dijkstra.min_y)), big)))
             for gx, gy in goals_xy]
    t = trace_paths(field, torch.tensor(cells, dtype=torch.int32, device=dev).reshape(-1, 3))
    origin = np.asarray(aabb.detach().cpu() if torch.is_tensor(aabb) else aabb, np.float64).reshape(-1)[:3]
    curves = min_snap_cells(t["paths"], t["offsets"], dijkstra.resolution, origin, height, yaw, v_avg)
    out = curves.sample(rate, min_samples, look_angles, False, max_samples, host)
    out.update({"curves": curves, "paths": t["paths"], "path_offsets": t["offsets"], "trace_info": t["info"]})
    if clearance is not None:
        c = clearance.trajectory_clearance(out["flat_x"], out["sample_offsets"], planner_axes=True, radius=radius)
        out["clearance"] = c
        out["certified"] = c["certified"] & (out["counts"] > 0)
    return out


class MinSnap:
    """planning/rotorpy/rotorpy/trajectories/minsnap.py's class: the same constructor, `initialize()`, `null`, `m`, `points`, `delta_t`,
    `t_keyframes`, `yaw_execute`, `x_poly`, `yaw_poly`, the derivative arrays and `update(t)`.  `from apnrf_amd.trajectory import MinSnap`
    replaces `from rotorpy.trajectories.minsnap import MinSnap`.  `initialize()` is one solve on the device and one copy of its result;
    `update` evaluates on the host as the reference does.  `initialize()` returns False where the status is not OK (see the module
    docstring); `status` holds it."""

    def __init__(self, points, yaw_angles=None, v_avg=2, device="cuda:0"):
        points = np.asarray(points, np.float64)
        self.yaw = np.zeros((points.shape[0])) if yaw_angles is None else yaw_angles
        self.v_avg = v_avg
        self.device = device
        self.full_points = points
        self.seg_dist = np.linalg.norm(np.diff(points, axis=0), axis=1)
        seg_mask = np.append(True, self.seg_dist > 1e-2)
        self.points = points[seg_mask, :]
        self.null = False
        self.status = None
        m = self.points.shape[0] - 1
        self.m = m
        self.x_dot_poly = np.zeros((m, 3, 7))
        self.x_ddot_poly = np.zeros((m, 3, 6))
        self.x_dddot_poly = np.zeros((m, 3, 5))
        self.x_ddddot_poly = np.zeros((m, 3, 4))
        self.yaw_dot_poly = np.zeros((m, 1, 7))
        self.yaw_ddot_poly = np.zeros((m, 1, 6))

    def initialize(self):
        m = self.m
        if self.points.shape[0] >= 2:
            curves = min_snap(self.full_points, None, (float(self.yaw[0]), float(self.yaw[-1])), self.v_avg, self.device)
            W = int(self.full_points.shape[0])
            packed = torch.cat([curves.coeffs.reshape(-1), curves.delta_t, curves.t_keyframes, curves.yaw_execute, curves.status.to(torch.float64),
                                curves.n_segments.to(torch.float64)]).cpu().numpy()
            self.status = int(packed[-2])
            if self.status != OK or int(packed[-1]) != m:
                return False
            self.delta_t = packed[32 * W:32 * W + m].copy()
            self.t_keyframes = packed[33 * W:33 * W + m + 1].copy()
            self.yaw_execute = packed[34 * W:34 * W + m + 1].copy()
            c = packed[:32 * m].reshape(m, 4, 8)
            self.x_poly = np.ascontiguousarray(c[:, :3, ::-1])                        # highest power first, as np.polyval reads them
            self.yaw_poly = np.ascontiguousarray(c[:, 3:, ::-1])
            self._derive()
            return True
        self.null = True
        self.status = NULL
        self.T = np.zeros((1,))
        self.x_poly = np.zeros((1, 3, 6))
        self.x_poly[0, :, -1] = self.full_points[0, :]
        return True

    def _derive(self):
        """The derivative polynomials, as np.polyder forms them from x_poly and yaw_poly."""
        for order, (xs, yaws) in enumerate(((self.x_dot_poly, self.yaw_dot_poly), (self.x_ddot_poly, self.yaw_ddot_poly), (self.x_dddot_poly, None),
                                            (self.x_ddddot_poly, None)), start=1):
            for i in range(self.m):
                xs[i] = [np.polyder(self.x_poly[i, j], m=order) for j in range(3)]
                if yaws is not None:
                    yaws[i, 0] = np.polyder(self.yaw_poly[i, 0], m=order)

    def update(self, t):
        """The flat outputs at time t, with the reference's keys; evaluated on the host from the copied coefficients."""
        out = {k: np.zeros((3,)) for k in ("x", "x_dot", "x_ddot", "x_dddot", "x_ddddot")}
        out.update(yaw=0, yaw_dot=0, yaw_ddot=0)
        if self.null:
            out["x"] = self.points[0, :]
            return out
        t = np.clip(t, self.t_keyframes[0], self.t_keyframes[-1])
        ends = self.t_keyframes[:-1] + self.delta_t                                   # the first segment whose end is not before t, else the last
        i = min(int(np.searchsorted(ends, t, side="left")), self.m - 1)
        tau = t - self.t_keyframes[i]
        for key, polys in (("x", self.x_poly), ("x_dot", self.x_dot_poly), ("x_ddot", self.x_ddot_poly), ("x_dddot", self.x_dddot_poly),
                           ("x_ddddot", self.x_ddddot_poly)):
            out[key] = np.array([np.polyval(polys[i, j], tau) for j in range(3)])
        for key, polys in (("yaw", self.yaw_poly), ("yaw_dot", self.yaw_dot_poly), ("yaw_ddot", self.yaw_ddot_poly)):
            out[key] = np.polyval(polys[i, 0], tau)
        return out
