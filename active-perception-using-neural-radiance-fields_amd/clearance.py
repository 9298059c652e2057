"""Trajectory clearance on the device (csrc/clearance.hip; include/mi355nerf.h "trajectory clearance"): how far a trajectory stays from
what the ensemble's occupancy grids call occupied, and which sample comes closest.

`clearance_field` turns level 0 of the members' `estimator.binaries` into a `ClearanceField`: the exact squared distance, in voxels, from
every voxel to the nearest voxel occupied in any member.  `ClearanceField.trajectory_clearance` looks samples up in it and forms
distances in metres, a sound lower bound, per-segment margins and a per-trajectory verdict; `ClearanceField.planner_map` inflates the
obstacles by a real radius over a height band for `Dijkstra` / `path_field`; `ClearanceField.sweep` walks the voxels of every segment.

The reference's own pieces (planning/planning_funcs.py) as drop-ins: `voxels_between_points` for get_voxels_between_points (:97-159),
`collision_checker` (:162-179), `world2voxels` (:187-189).  Their quirks are the reference's and are kept (the header lists them).

LIMITS.  Level 0 of the estimator only; axes up to 2048 voxels; cubic voxels.  `lower` is sound but loose by sqrt(3) voxels: a sample
anywhere in its voxel and an obstacle anywhere in its voxel are at least (sqrt(d2) - sqrt(3)) voxel edges apart."""
import ctypes
import math

import numpy as np
import torch

from . import _lib as L

INT32_MAX = 0x7FFFFFFF
SQRT3 = math.sqrt(3.0)
MAX_AXIS = 2048
DEFAULT_MAX_STEPS = 1 << 16


def d2_threshold(radius, voxel):
    """floor((radius / voxel + sqrt(3) / 2)^2): the `d2_max` for `ClearanceField.planner_map`.  A vehicle centred ANYWHERE in a voxel
    whose d2 is larger than this is farther than `radius` from the centre of every occupied voxel: its own voxel's centre is at
    least sqrt(d2) voxel edges from theirs, and it is at most half a voxel diagonal from its own."""
    return int(math.floor((float(radius) / float(voxel) + SQRT3 / 2) ** 2))


def _u8_grids(b):
    if not torch.is_tensor(b):
        h = np.ascontiguousarray(np.asarray(b))
        b = torch.from_numpy(h if h.flags.writeable else h.copy())
    if b.dim() == 3:
        b = b[None]
    if b.dim() != 4:
        raise ValueError(f"binaries is [X,Y,Z] or [members,X,Y,Z] (got {tuple(b.shape)})")
    if b.dtype == torch.bool:
        return b.contiguous().view(torch.uint8)
    return (b != 0).to(torch.uint8).contiguous() if b.dtype != torch.uint8 else b.contiguous()


def _f64(a, device):
    t = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64)))
    return L.contig(t.to(device), torch.float64)


def _i32(a, device):
    t = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(np.asarray(a)))
    return L.contig(t.to(device), torch.int32)


def _check_axes(shape):
    if any(int(n) < 1 or int(n) > MAX_AXIS for n in shape[-3:]) or int(np.prod([int(n) for n in shape[-3:]])) > (1 << 31) - 64:
        raise L.MnfError(f"a {tuple(int(n) for n in shape[-3:])} grid is outside what a clearance field holds: axes 1 .. {MAX_AXIS}, < 2^31 - 64 voxels")


@torch.no_grad()
def clearance_field(binaries_or_estimators, aabb=None, voxel=None, device=None):
    """-> ClearanceField.  Either a list of estimators (level 0 of each one's `binaries`; the aabb is the first one's `aabbs[0]`), or
    a uint8 / bool array [members,X,Y,Z] (or [X,Y,Z]) with `aabb` = (x0, y0, z0, x1, y1, z1) in the grid's axis order.  `voxel` is the
    edge the voxel indices are formed with (the reference's `voxel_grid_size`, 0.2 in the yaml); None takes (x1 - x0) / X, which may
    differ from the intended decimal by an ulp and then places a sample that lies on a voxel face differently.  One launch sequence on
    the device; the grids are not copied to the host."""
    src = binaries_or_estimators
    if isinstance(src, (list, tuple)) and src and hasattr(src[0], "binaries"):
        grids = torch.stack([e.binaries[0] for e in src])
        if aabb is None:
            aabb = src[0].aabbs[0]
    elif hasattr(src, "binaries"):
        grids = src.binaries[0][None]
        if aabb is None:
            aabb = src.aabbs[0]
    else:
        grids = src
    if aabb is None:
        raise ValueError("an array of grids needs its aabb")
    grids = _u8_grids(grids)
    if device is not None:
        grids = grids.to(device)
    L.require_gpu(grids)
    _check_axes(grids.shape)
    a = np.asarray(aabb.detach().cpu().numpy() if torch.is_tensor(aabb) else aabb, np.float64).reshape(6)
    M, X, Y, Z = (int(v) for v in grids.shape)
    edges = (a[3:] - a[:3]) / np.array([X, Y, Z], np.float64)
    if not (np.isfinite(edges).all() and (edges > 0).all()):
        raise ValueError(f"aabb {a.tolist()} is empty or not finite")
    if edges.max() - edges.min() > 1e-6 * edges.max():
        raise ValueError(f"distances in voxels need cubic voxels (edges {edges.tolist()})")
    if voxel is None:
        voxel = float(edges[0])
    elif not (math.isfinite(float(voxel)) and abs(float(voxel) - edges[0]) <= 1e-6 * edges[0]):
        raise ValueError(f"voxel {voxel} is not the edge of {X} x {Y} x {Z} voxels over aabb {a.tolist()} ({edges[0]})")
    d2 = torch.empty(X, Y, Z, dtype=torch.int32, device=grids.device)
    info = torch.empty(2, dtype=torch.int64, device=grids.device)
    L.launch(L.load_library().mnf_clearance_field, L.ptr(grids), M, X, Y, Z, L.ptr(d2), L.ptr(info))
    return ClearanceField(d2, info, a, float(voxel), grids)


def _traj_of_points(offsets, n_points):
    """int64 [P]: the trajectory that holds each point (torch, on the device)."""
    idx = torch.arange(n_points, device=offsets.device, dtype=torch.int64)
    return torch.searchsorted(offsets[1:].contiguous(), idx, right=True)


class ClearanceField:
    """`d2` int32 [X,Y,Z] (0 on occupied voxels, INT32_MAX everywhere for an empty map), `info` int64 [2] = {occupied voxels, largest
    finite d2 or -1}, `aabb` float64 [6], `voxel` float64 scalar: device tensors.  `binaries` uint8 [members,X,Y,Z] is the input, kept for
    `sweep`."""

    def __init__(self, d2, info, aabb_host, voxel_host, binaries):
        self.d2, self.info, self.binaries = d2, info, binaries
        self.device = d2.device
        self._aabb = np.asarray(aabb_host, np.float64).reshape(6)
        self._voxel = float(voxel_host)
        self.aabb = torch.from_numpy(self._aabb.copy()).to(self.device)
        self.voxel = torch.tensor(self._voxel, dtype=torch.float64, device=self.device)
        self._origin_c = (ctypes.c_double * 3)(*[float(v) for v in self._aabb[:3]])

    @property
    def shape(self):
        return tuple(int(v) for v in self.d2.shape)

    def _points(self, points, offsets, planner_axes):
        p = _f64(points, self.device).reshape(-1, 3)
        if planner_axes:
            p = p[:, [0, 2, 1]].contiguous()                                           # sample_traj's x, z, y -> the estimator's x, y, z
        P = int(p.shape[0])
        if offsets is None:
            off = torch.tensor([0, P], dtype=torch.int64, device=self.device)
        else:
            off = offsets if torch.is_tensor(offsets) else torch.from_numpy(np.ascontiguousarray(np.asarray(offsets, np.int64)))
            off = L.contig(off.to(self.device), torch.int64).reshape(-1)
            if int(off.shape[0]) < 1:
                raise ValueError("offsets is [T+1]")
        return p, off, P

    @torch.no_grad()
    def lookup(self, points, offsets=None, planner_axes=False):
        """The kernel's integers: {"cells" int32 [P,3], "point_d2" int32 [P] (-1 outside the grid or not finite), "traj" int64 [T,4] =
        {least d2 or -1, index within the trajectory of the first sample attaining it, samples outside, samples}, "info" int64 [2] =
        {samples outside, samples not finite}, "points" float64 [P,3] in the grid's axis order, "offsets" int64 [T+1]}."""
        p, off, P = self._points(points, offsets, planner_axes)
        T = int(off.shape[0]) - 1
        X, Y, Z = self.shape
        cells = torch.empty(P, 3, dtype=torch.int32, device=self.device)
        pd2 = torch.full((P,), -1, dtype=torch.int32, device=self.device)
        traj = torch.empty(T, 4, dtype=torch.int64, device=self.device)
        info = torch.zeros(2, dtype=torch.int64, device=self.device)
        L.launch(L.load_library().mnf_clearance_lookup, L.ptr(self.d2), X, Y, Z, self._origin_c, self._voxel, L.ptr(p) if P else None, P, L.ptr(off), T,
                 L.ptr(cells) if P else None, L.ptr(pd2) if P else None, L.ptr(traj) if T else None, L.ptr(info))
        return {"cells": cells, "point_d2": pd2, "traj": traj, "info": info, "points": p, "offsets": off}

    @torch.no_grad()
    def trajectory_clearance(self, points, offsets=None, planner_axes=False, radius=0.0, host=False):
        """`points` [P,3] (device or host) packed at `offsets` [T+1] (None: one trajectory); `planner_axes=True` takes sample_traj's
        x, z, y order.  -> the integers of `lookup` and, formed from them with torch on the device in float64:
          "metres" [P]  sqrt(d2) * voxel, voxel centre to voxel centre (NaN for a sample outside, inf for an empty map);
          "lower"  [P]  max(0, sqrt(d2) - sqrt(3)) * voxel: no obstacle voxel comes nearer to the sample than this (0 outside);
          "margin" [P]  entry i is the segment from sample i to i + 1: (lower_i + lower_{i+1} - |p_{i+1} - p_i|) / 2, a clearance every
                        point of the segment has; +inf where sample i ends its trajectory, and the sample's own `lower` where it is
                        the trajectory's only one;
          "certified" [T] bool: every margin of the trajectory > radius and no sample outside;
          "closest" [T] the least `metres` of the trajectory (NaN when no sample is inside).
        Nothing is copied to the host unless `host=True`, which adds "summary": traj and certified as numpy arrays, in one copy."""
        out = self.lookup(points, offsets, planner_axes)
        p, off, pd2, traj = out["points"], out["offsets"], out["point_d2"], out["traj"]
        P, T = int(p.shape[0]), int(traj.shape[0])
        inside = pd2 >= 0
        root = torch.sqrt(pd2.clamp(min=0).to(torch.float64))
        nan = torch.full_like(root, float("nan"))
        metres = torch.where(inside, root * self.voxel, nan)
        lower = torch.where(inside, (root - SQRT3).clamp(min=0.0) * self.voxel, torch.zeros_like(root))
        margin = torch.full((P,), float("inf"), dtype=torch.float64, device=self.device)
        certified = traj[:, 2] == 0
        if P:
            tid = _traj_of_points(off, P)
            if P > 1:
                d = p[1:] - p[:-1]
                length = torch.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
                seg = ((lower[:-1] + lower[1:]) - length) / 2
                margin[:-1] = torch.where(tid[:-1] == tid[1:], seg, margin[:-1])
            covered = tid < T
            tid_c = tid.clamp(max=max(T - 1, 0))
            if T:
                single = covered & (traj[tid_c, 3] == 1)
                margin = torch.where(single, lower, margin)
                ok = torch.ones(T, dtype=torch.int32, device=self.device)
                bad = covered & ~(margin > radius)
                ok.scatter_reduce_(0, tid_c, (~bad).to(torch.int32), reduce="amin", include_self=True)
                certified = certified & (ok == 1)
        root_t = torch.sqrt(traj[:, 0].clamp(min=0).to(torch.float64)) * self.voxel
        closest = torch.where(traj[:, 0] >= 0, root_t, torch.full_like(root_t, float("nan")))
        out.update({"metres": metres, "lower": lower, "margin": margin, "certified": certified, "closest": closest})
        if host:
            packed = torch.cat([traj, certified.to(torch.int64)[:, None]], dim=1).cpu().numpy()
            out["summary"] = {"traj": packed[:, :4], "certified": packed[:, 4].astype(bool)}
        return out

    @torch.no_grad()
    def planner_map(self, y_lo, y_hi, d2_max):
        """int32 device tensor [X,Z]: 1 where any voxel of the height band y_lo <= y < y_hi has d2 <= d2_max (`d2_threshold(radius,
        voxel)` for a vehicle radius), else 0.  What `Dijkstra` / `path_field` take as it stands."""
        X, Y, Z = self.shape
        y_lo, y_hi = int(y_lo), int(y_hi)
        if not 0 <= y_lo < y_hi <= Y:
            raise ValueError(f"the height band [{y_lo}, {y_hi}) is outside [0, {Y}]")
        return (self.d2[:, y_lo:y_hi, :] <= int(d2_max)).any(dim=1).to(torch.int32).contiguous()

    @torch.no_grad()
    def sweep(self, points, offsets=None, members=None, planner_axes=False, max_steps=DEFAULT_MAX_STEPS):
        """The voxel walk of every segment of every trajectory, in ONE frame: positions relative to the aabb's origin, voxels from the
        same positions.  `members`: indices of the grids to read (None: all).  -> {"hits" int32 [P,5], row i the segment from sample i
        to i + 1 = {position in the walk of the first occupied voxel or -1, its three indices, walk length}; rows of samples that end a
        trajectory are (-1, -1, -1, -1, 0); "segment" bool [P]; "info" int64 [3] = {walks cut at max_steps, walks not finite, 0}}."""
        look = self.lookup(points, offsets, planner_axes)
        p, off, cells = look["points"], look["offsets"], look["cells"]
        P = int(p.shape[0])
        grids = self.binaries if members is None else self.binaries[torch.as_tensor(list(members), device=self.device, dtype=torch.int64)].contiguous()
        hits = torch.full((P, 5), -1, dtype=torch.int32, device=self.device)
        hits[:, 4] = 0
        info = torch.zeros(3, dtype=torch.int64, device=self.device)
        segment = torch.zeros(P, dtype=torch.bool, device=self.device)
        if P > 1 and int(grids.shape[0]) > 0:
            tid = _traj_of_points(off, P)
            segment[:-1] = (tid[:-1] == tid[1:]) & (tid[:-1] < int(off.shape[0]) - 1)
            rel = p - self.aabb[:3]
            # a pair that straddles two trajectories is no segment: its start is made NaN, so its walk has length 0 and the row
            # (-1, -1, -1, -1, 0); the kernel counts it as not finite, which is taken off again where the pair itself was finite
            seg = segment[:-1]
            finite = torch.isfinite(rel[:-1]).all(dim=1) & torch.isfinite(rel[1:]).all(dim=1)
            starts = torch.where(seg[:, None], rel[:-1], torch.full_like(rel[:-1], float("nan")))
            raw = walk_hits(starts, rel[1:], cells[:-1], cells[1:], self._voxel, grids, max_steps=max_steps)
            hits[:-1] = raw["hits"]
            info = raw["info"]
            info[1] -= (~seg & finite).sum()
        return {"hits": hits, "segment": segment, "info": info}


def _walk_inputs(start, end, current_voxel, end_voxel, device):
    s, e = _f64(start, device).reshape(-1, 3), _f64(end, device).reshape(-1, 3)
    c, v = _i32(current_voxel, device).reshape(-1, 3), _i32(end_voxel, device).reshape(-1, 3)
    L.require_gpu(s, e, c, v)
    n = int(s.shape[0])
    if not (int(e.shape[0]) == int(c.shape[0]) == int(v.shape[0]) == n):
        raise ValueError("start, end, current_voxel and end_voxel are [n,3] with one n")
    return s, e, c, v, n


@torch.no_grad()
def voxel_walks(start, end, current_voxel, end_voxel, voxel_size, max_steps=DEFAULT_MAX_STEPS, device="cuda:0"):
    """get_voxels_between_points for n chords at once: count, offsets, fill.  -> {"voxels" int32 [total,3] packed at "offsets" int64
    [n+1], "counts" int64 [n], "info" int64 [3] = {walks cut at max_steps, walks not finite, slots that did not match}}: device
    tensors; the total is the one host read."""
    dev = start.device if torch.is_tensor(start) and start.is_cuda else torch.device(device)
    s, e, c, v, n = _walk_inputs(start, end, current_voxel, end_voxel, dev)
    lib = L.load_library()
    counts = torch.empty(n, dtype=torch.int64, device=dev)
    info = torch.zeros(3, dtype=torch.int64, device=dev)
    scratch = torch.zeros(3, dtype=torch.int64, device=dev)
    L.launch(lib.mnf_voxel_walk_count, L.ptr(s) if n else None, L.ptr(e) if n else None, L.ptr(c) if n else None, L.ptr(v) if n else None, n,
             float(voxel_size), int(max_steps), L.ptr(counts) if n else None, L.ptr(info), device=dev)
    offsets = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    offsets[1:] = torch.cumsum(counts, 0)
    total = int(offsets[-1].item()) if n else 0
    voxels = torch.empty(max(total, 1), 3, dtype=torch.int32, device=dev)
    L.launch(lib.mnf_voxel_walk_fill, L.ptr(s) if n else None, L.ptr(e) if n else None, L.ptr(c) if n else None, L.ptr(v) if n else None, n,
             float(voxel_size), int(max_steps), L.ptr(offsets), total, L.ptr(voxels), L.ptr(scratch), device=dev)
    info[2] = scratch[2]                                                                # cut and not-finite walks were counted once already
    return {"voxels": voxels[:total], "offsets": offsets, "counts": counts, "info": info}


@torch.no_grad()
def walk_hits(start, end, current_voxel, end_voxel, voxel_size, binaries, max_steps=DEFAULT_MAX_STEPS, info=None):
    """The first occupied voxel of n walks without building their lists.  `binaries` uint8 / bool [members,X,Y,Z] (or [X,Y,Z]) on the
    device: a voxel counts when any of them holds it, every index clipped to the grid first.  -> {"hits" int32 [n,5], "info" int64 [3]}."""
    grids = _u8_grids(binaries)
    L.require_gpu(grids)
    _check_axes(grids.shape)
    dev = grids.device
    s, e, c, v, n = _walk_inputs(start, end, current_voxel, end_voxel, dev)
    M, X, Y, Z = (int(k) for k in grids.shape)
    hits = torch.empty(n, 5, dtype=torch.int32, device=dev)
    info = torch.zeros(3, dtype=torch.int64, device=dev) if info is None else info
    L.launch(L.load_library().mnf_voxel_walk_hits, L.ptr(s) if n else None, L.ptr(e) if n else None, L.ptr(c) if n else None, L.ptr(v) if n else None, n,
             float(voxel_size), int(max_steps), L.ptr(grids), M, X, Y, Z, L.ptr(hits) if n else None, L.ptr(info), device=dev)
    return {"hits": hits, "info": info}


def world2voxels(x, voxel_grid_size=0.1):
    """planning_funcs.py:187-189 on the host, as it stands there: numpy's float64 floor_divide and the cast to int."""
    return np.array(np.asarray(x) // voxel_grid_size, dtype=int)


def voxels_between_points(start_pos, end_pose, current_voxel, end_voxel, voxel_size, max_steps=DEFAULT_MAX_STEPS, device="cuda:0"):
    """get_voxels_between_points (planning_funcs.py:97-159) with its signature and its result: a list of int32 arrays [3], the start
    voxel not among them.  A walk cut at `max_steps` raises: the list would not be the reference's."""
    out = voxel_walks(np.asarray(start_pos, np.float64).reshape(1, 3), np.asarray(end_pose, np.float64).reshape(1, 3),
                      np.asarray(current_voxel).astype(np.int32).reshape(1, 3), np.asarray(end_voxel).astype(np.int32).reshape(1, 3), voxel_size,
                      max_steps=max_steps, device=device)
    info = out["info"].cpu().numpy()
    if info[0] or info[2]:
        raise L.MnfError(f"the voxel walk was cut at max_steps = {max_steps}")
    return [row.copy() for row in out["voxels"].cpu().numpy()]


def collision_checker(voxel_grid, flat, voxel_grid_size, aabb, max_steps=DEFAULT_MAX_STEPS, device="cuda:0"):
    """planning_funcs.py:162-179 as a drop-in: the chord from the first to the last sample of flat["x"], positions in world coordinates
    and voxels in the aabb's frame (the reference's own mix), member 0 of `voxel_grid` [members,X,Y,Z] (host or device), every index
    clipped to the grid.  Returns the same bool and prints nothing.  One launch; the bool is the one host read."""
    x = np.asarray(flat["x"].detach().cpu().numpy() if torch.is_tensor(flat["x"]) else flat["x"], np.float64)
    origin = np.asarray(aabb.detach().cpu().numpy() if torch.is_tensor(aabb) else aabb, np.float64).reshape(-1)[:3]
    idx = world2voxels(x[[0, -1]] - origin, voxel_grid_size)
    idx = np.clip(idx, -(1 << 30), 1 << 30).astype(np.int32)
    g = voxel_grid if torch.is_tensor(voxel_grid) else torch.from_numpy(np.ascontiguousarray(np.asarray(voxel_grid)))
    g = g[0] if g.dim() == 4 else g
    if not g.is_cuda:
        g = g.to(device)
    out = walk_hits(x[0].reshape(1, 3), x[-1].reshape(1, 3), idx[0].reshape(1, 3), idx[1].reshape(1, 3), voxel_grid_size, g, max_steps=max_steps)
    return bool(out["hits"][0, 0].item() >= 0)
