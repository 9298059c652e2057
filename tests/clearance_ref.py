"""numpy restatement of the trajectory-clearance unit (csrc/clearance.hip, include/mi355nerf.h "trajectory clearance"): numpy's float64
floor_divide spelt out, the voxel of a point, the reference's voxel walk (planning/planning_funcs.py:97-159), collision_checker's clipped
look-up (:162-179), a brute-force squared distance field, and the lookup of trajectory samples.  tests/test_clearance_cpu.py holds the
walk, the floor division and the checker to the reference's own answers (tests/golden/clearance_walks.npz); the GPU tests compare the
device with this file."""
import math

import numpy as np

INT32_MAX = 0x7FFFFFFF
INT32_MIN = -0x80000000
CELL_FAR = 1 << 30
SQRT3 = math.sqrt(3.0)


# ------------------------------------------------------------------ the voxel of a point
def floor_divide(a, b):
    """npy_divmod's quotient for two Python floats, without using `//`: the exact remainder, the sign fix, the round-up."""
    a, b = float(a), float(b)
    if b == 0.0:
        return math.nan if (a == 0.0 or a != a) else math.copysign(math.inf, a) * math.copysign(1.0, b)
    if math.isinf(a) or a != a or b != b:
        return math.nan
    mod = math.fmod(a, b)                                       # exact; for an infinite b it is a
    div = (a - mod) / b
    if mod != 0.0 and ((b < 0.0) != (mod < 0.0)):
        div -= 1.0
    if div != 0.0:
        fl = math.floor(div) if math.isfinite(div) else div
        if div - fl > 0.5:
            fl += 1.0
        return float(fl)
    return math.copysign(0.0, a / b)


def cell_of(q):
    if not math.isfinite(q):
        return INT32_MIN
    return int(min(max(q, -float(CELL_FAR)), float(CELL_FAR)))


def world2voxels(x, size):
    """int32 [...,3]: the reference's world2voxels(x, size) for x already relative to the grid's origin."""
    x = np.asarray(x, np.float64)
    out = np.empty(x.shape, np.int32)
    flat, o = x.reshape(-1), out.reshape(-1)
    for i in range(flat.shape[0]):
        o[i] = cell_of(floor_divide(flat[i], size))
    return out


def cells_of_points(points, origin, size):
    p = np.asarray(points, np.float64).reshape(-1, 3)
    with np.errstate(invalid="ignore", over="ignore"):
        rel = p - np.asarray(origin, np.float64).reshape(1, 3)
    return world2voxels(rel, size)


# ------------------------------------------------------------------ the voxel walk
def voxel_walk(start_pos, end_pos, current_voxel, end_voxel, voxel_size, max_steps=1 << 20):
    """-> (int32 [len,3], cut, finite): get_voxels_between_points statement by statement, bounded by max_steps; a start or end that is
    not finite gives no voxel."""
    s = np.asarray(start_pos, np.float64).reshape(3)
    e = np.asarray(end_pos, np.float64).reshape(3)
    if not (np.isfinite(s).all() and np.isfinite(e).all()):
        return np.zeros((0, 3), np.int32), False, False
    size = np.float64(voxel_size)
    cur = np.asarray(current_voxel).astype(np.int32).reshape(3).copy()
    view = cur.copy()
    last = np.asarray(end_voxel).astype(np.int32).reshape(3)
    ray = e - s
    step = np.where(ray >= 0, 1.0, -1.0)
    nxt = (cur + step) * size
    t_max = np.full(3, np.inf)
    t_delta = np.full(3, np.inf)
    with np.errstate(all="ignore"):
        for i in range(3):
            if ray[i] != 0:
                t_max[i] = (nxt[i] - s[i]) / ray[i]
                t_delta[i] = size / ray[i] * step[i]

        def dist_of(v):
            d = (v - view).astype(np.int32) * size              # the int32 difference wraps as numpy's does
            sq = d * d
            return (sq[0] + sq[1]) + sq[2]

        range_sq = dist_of(last)
        dist = dist_of(cur)
        out = []
        cut = False
        while dist <= range_sq:
            if len(out) >= max_steps:
                cut = True
                break
            if t_max[0] < t_max[1]:
                a = 0 if t_max[0] < t_max[2] else 2
            else:
                a = 1 if t_max[1] < t_max[2] else 2
            cur[a] = np.int32(cur[a]) + np.int32(step[a])
            t_max[a] += t_delta[a]
            out.append(cur.copy())
            dist = dist_of(cur)
    return np.array(out, np.int32).reshape(-1, 3), cut, True


def walk_hit(voxels, grids):
    """int32 [5]: {position of the first listed voxel occupied in any grid of `grids` [M,X,Y,Z] after clipping, or -1; its three indices
    as listed; the length of the list}."""
    g = np.asarray(grids)
    any_occ = g if (g.ndim == 3 and g.dtype == np.bool_) else (g != 0).any(axis=0)   # a finished bool union [X,Y,Z] is taken as it is
    row = np.array([-1, -1, -1, -1, voxels.shape[0]], np.int32)
    if voxels.shape[0]:
        c = [np.clip(voxels[:, k], 0, any_occ.shape[k] - 1) for k in range(3)]
        occ = any_occ[c[0], c[1], c[2]]
        if occ.any():
            k = int(np.argmax(occ))
            row[:4] = [k, voxels[k, 0], voxels[k, 1], voxels[k, 2]]
    return row


def collision_checker(voxel_grid, x, voxel_grid_size, aabb):
    """The reference's collision_checker on flat["x"] = x: the chord of the first and last sample in world coordinates, the voxels in the
    aabb's frame, member 0."""
    x = np.asarray(x, np.float64)
    idx = world2voxels(x[[0, -1]] - np.asarray(aabb, np.float64)[:3], voxel_grid_size)
    vox, _, _ = voxel_walk(x[0], x[-1], idx[0], idx[1], voxel_grid_size)
    return bool(walk_hit(vox, np.asarray(voxel_grid)[:1])[0] >= 0)


# ------------------------------------------------------------------ the field and the lookup
def brute_d2(binaries):
    """int32 [X,Y,Z]: the squared distance in voxels to the nearest voxel occupied in any member, by comparing every voxel with every
    occupied one; INT32_MAX everywhere for an empty union.  -> (d2, info [2])."""
    b = np.asarray(binaries)
    occ = (b != 0).any(axis=0) if b.ndim == 4 else b != 0
    shape = occ.shape
    pts = np.argwhere(occ).astype(np.int64)
    if pts.shape[0] == 0:
        return np.full(shape, INT32_MAX, np.int32), np.array([0, -1], np.int64)
    grid = np.stack(np.meshgrid(*[np.arange(n, dtype=np.int64) for n in shape], indexing="ij"), axis=-1).reshape(-1, 3)
    best = np.full(grid.shape[0], np.iinfo(np.int64).max, np.int64)
    for lo in range(0, pts.shape[0], 256):
        d = grid[:, None, :] - pts[None, lo:lo + 256, :]
        best = np.minimum(best, (d * d).sum(axis=2).min(axis=1))
    d2 = best.reshape(shape).astype(np.int32)
    return d2, np.array([pts.shape[0], int(d2.max())], np.int64)


def lookup(d2, origin, voxel, points, offsets):
    """-> (cells [P,3] int32, point_d2 [P] int32, traj [T,4] int64, info [2] int64) as mnf_clearance_lookup defines them."""
    d2 = np.asarray(d2)
    p = np.asarray(points, np.float64).reshape(-1, 3)
    offsets = np.asarray(offsets, np.int64)
    cells = cells_of_points(p, origin, voxel)
    finite = np.isfinite(p).all(axis=1)
    inside = finite & (cells >= 0).all(axis=1) & (cells < np.array(d2.shape)).all(axis=1)
    pd2 = np.full(p.shape[0], -1, np.int32)
    ci = cells[inside]
    pd2[inside] = d2[ci[:, 0], ci[:, 1], ci[:, 2]]
    T = offsets.shape[0] - 1
    traj = np.zeros((T, 4), np.int64)
    info = np.zeros(2, np.int64)
    for t in range(T):
        a, b = int(offsets[t]), int(offsets[t + 1])
        v, ins = pd2[a:b], inside[a:b]
        traj[t, 2], traj[t, 3] = int((~ins).sum()), b - a
        if ins.any():
            m = int(v[ins].min())
            traj[t, 0], traj[t, 1] = m, int(np.argmax(ins & (v == m)))
        else:
            traj[t, 0] = traj[t, 1] = -1
        info[0] += traj[t, 2]
        info[1] += int((~finite[a:b]).sum())
    return cells, pd2, traj, info


# ------------------------------------------------------------------ the float64 values apnrf_amd.clearance forms from the integers
def metres_lower(point_d2, voxel):
    d = np.sqrt(np.maximum(np.asarray(point_d2), 0).astype(np.float64))
    return d * voxel, np.maximum(0.0, d - SQRT3) * voxel


def d2_threshold(radius, voxel):
    return int(math.floor((radius / voxel + SQRT3 / 2) ** 2))
