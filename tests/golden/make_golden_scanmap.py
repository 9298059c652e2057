"""Writes tests/golden/scan_maps.npz: what the reference's own `update_cost_map` (planning/planning_funcs.py:192-219, over
perception/data_proc/depth_to_grid.py) leaves in cost_map and the summed visiting_map, view after view, driven as
scripts/pipeline.py:272-292 drives it.

    python tests/golden/make_golden_scanmap.py --reference /path/to/the/reference/tree

The reference modules are imported at generation time only (what they import and this container lacks is placeholdered, as
ref_shim.py does); scipy gives the yaw values.  The fixture holds data: depth images, poses, align angles, aabb, resolution, and per
view the yaw, the centre cell and the reference's two maps.  The generator asserts, on the reference's answers alone, that the fixture
holds the cases the tests rely on, and prints the host time of the reference's loop for 6 and 39 views of 640 beams on a 98 x 98 map."""
import argparse
import os
import sys
import time
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import scanmap_ref as SR  # noqa: E402  (input preparation only: settle_depths)


class _Anything(types.ModuleType):
    """A placeholder module: any attribute is a further placeholder (the planner's simulator imports are never called here)."""

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return lambda *a, **k: None


def _placeholder(name):
    try:
        __import__(name)
    except Exception:
        parts = name.split(".")
        for i in range(1, len(parts) + 1):
            sys.modules.setdefault(".".join(parts[:i]), _Anything(".".join(parts[:i])))


def import_reference(root):
    sys.path.insert(0, os.path.join(root, "planning"))
    sys.path.insert(0, os.path.join(root, "perception", "data_proc"))
    for name in ("rotorpy.vehicles.multirotor", "rotorpy.vehicles.crazyflie_params", "rotorpy.controllers.quadrotor_control",
                 "rotorpy.trajectories.minsnap", "rotorpy.simulate", "tqdm", "matplotlib", "matplotlib.pyplot"):
        _placeholder(name)
    import depth_to_grid
    import planning_funcs
    return planning_funcs, depth_to_grid


def align_of(width):
    half = width // 2                                                                 # pipeline.py:227-230 with 320 -> half
    r = np.arctan(np.linspace(0.5, half - 0.5, half) / half).tolist()
    r.reverse()
    l = np.arctan(-np.linspace(0.5, half - 0.5, half) / half).tolist()
    return np.array(r + l)


def make_poses(rng, n, x_range, z_range, y):
    from scipy.spatial.transform import Rotation as R
    poses = []
    for i in range(n):
        ang = [rng.uniform(-np.pi, np.pi), rng.uniform(-0.25, 0.25), rng.uniform(-0.25, 0.25)]
        T = np.eye(4)
        T[:3, :3] = R.from_euler("yzx", ang).as_matrix()
        T[:3, 3] = [rng.uniform(*x_range), y, rng.uniform(*z_range)]
        poses.append(T)
    return np.array(poses)


def make_depth(rng, V, H, W, lo, hi):
    th = np.linspace(0, 2 * np.pi, W)
    d = np.empty((V, H, W), np.float32)
    for v in range(V):
        base = 0.5 * (lo + hi) + 0.3 * (hi - lo) * np.sin(3 * th + rng.uniform(0, 6))
        row = np.clip(base + rng.uniform(-0.25, 0.25, W) * (hi - lo), lo, hi)
        d[v] = rng.uniform(lo, hi, (H, W))                                            # the other rows are never read
        d[v, H // 2] = row
    return d


def run_reference(PF, DG, depth, poses, align, aabb32, res, shape):
    """pipeline.py:272-292, with the reference's functions recorded on the way."""
    from scipy.spatial.transform import Rotation as R
    rec = {"coords": [], "cells": [], "orders": [0, 0]}
    real_grid, real_bres = PF.generate_ray_casting_grid_map, DG.bresenham

    def grid_spy(ox, oy, x_w, y_w, loc_x, loc_y, aabb, xy_resolution, breshen=True):
        fx, fy = (np.asarray(ox) - aabb[2]) / xy_resolution, (np.asarray(oy) - aabb[0]) / xy_resolution
        rec["coords"].append((fx, fy))
        state = {}                                                                    # cell -> (occupied?, beam)
        beams = []
        DG.bresenham = lambda s, e: beams.append(real_bres(s, e)) or beams[-1]
        out = real_grid(ox, oy, x_w, y_w, loc_x, loc_y, aabb, xy_resolution, breshen)
        DG.bresenham = real_bres
        assert len(beams) == len(fx)
        for j, cells in enumerate(beams):
            rec["cells"].append(cells)
            ix, iy = int(round(fx[j])), int(round(fy[j]))
            assert tuple(cells[0]) == (loc_x, loc_y) or tuple(cells[-1]) == (loc_x, loc_y)
            for c in map(tuple, cells):
                if state.get(c, (False, j))[0] and state[c][1] < j:
                    rec["orders"][0] += 1                                             # occupied by an earlier beam, freed by this one
                state[c] = (False, j)
            for c in ((ix, iy), (ix + 1, iy), (ix, iy + 1), (ix + 1, iy + 1)):
                if c in state and not state[c][0] and state[c][1] < j:
                    rec["orders"][1] += 1                                             # freed by an earlier beam, occupied by this one
                state[c] = (True, j)
        return out

    PF.generate_ray_casting_grid_map = grid_spy
    cost_map, visiting = np.full(shape, 0.5), np.zeros(shape)
    yaws, centres, costs, visits = [], [], [], []
    for i, d_img in enumerate(depth):
        d_points = d_img[int(d_img.shape[0] / 2)]
        euler = R.from_matrix(poses[i][:3, :3]).as_euler("yzx")
        assert abs(abs(euler[1]) - np.pi / 2) > 1.0                                   # pitch and roll away from the Euler singularity
        d_angles = (align + euler[0]) % (2 * np.pi)
        w_loc = poses[i][:3, 3]
        grid_loc = np.array((w_loc - aabb32[:3]) // res, dtype=int)
        cost_map, visiting_map = PF.update_cost_map(cost_map=cost_map, depth=d_points, angle=d_angles, g_loc=grid_loc, w_loc=w_loc, aabb=aabb32,
                                                    resolution=res)
        visiting += visiting_map
        yaws.append(euler[0]); centres.append([grid_loc[0], grid_loc[2]])
        costs.append(cost_map.copy()); visits.append(visiting.copy())
    PF.generate_ray_casting_grid_map = real_grid
    return np.array(yaws), np.array(centres, np.int32), np.array(costs), np.array(visits), rec


def make_case(PF, DG, rng, shape, res, origin, V, H, W, cam_x, cam_z, depth_range):
    nx, nz = shape
    aabb32 = np.array([origin[0], -0.5, origin[1], origin[0] + nx * res + 1e-3, 2.5, origin[1] + nz * res + 1e-3], np.float32)
    assert aabb32[0] != aabb32[2] and nx != nz
    align = align_of(W)
    poses = make_poses(rng, V, cam_x, cam_z, 1.2)
    depth = make_depth(rng, V, H, W, *depth_range)
    from scipy.spatial.transform import Rotation as R
    yaw0 = np.array([R.from_matrix(p[:3, :3]).as_euler("yzx")[0] for p in poses])
    depth[:, H // 2] = SR.settle_depths(depth[:, H // 2], align, yaw0, poses[:, [0, 2], 3], aabb32.astype(np.float64), res)
    yaws, centres, costs, visits, rec = run_reference(PF, DG, depth, poses, align, aabb32, res, shape)
    # the fixture's conditions, on the reference's answers alone
    for fx, fy in rec["coords"]:
        assert (np.abs(fx - np.floor(fx) - 0.5) > 1e-6).all() and (np.abs(fy - np.floor(fy) - 0.5) > 1e-6).all()
    assert all((c >= 0).all() for c in rec["cells"]) and all(min(np.rint(fx).min(), np.rint(fy).min()) >= 0 for fx, fy in rec["coords"])
    assert rec["orders"][0] > 0 and rec["orders"][1] > 0, rec["orders"]
    changed = sum(int(((costs[v] != costs[v - 1]) & (costs[v - 1] != 0.5)).sum()) for v in range(1, V))
    assert changed > 0
    high = sum(int((c[:, 0] >= nx).sum() + (c[:, 1] >= nz).sum()) for c in rec["cells"])
    print(f"{nx} x {nz}, {V} views of {W} beams: {rec['orders'][0]} occupied-then-freed, {rec['orders'][1]} freed-then-occupied, "
          f"{changed} cells changed by a later view, {high} cells beyond the high side")
    return dict(aabb=aabb32, res=np.float64(res), shape=np.array(shape, np.int32), align=align, poses=poses, depth=depth, yaw=yaws, centre=centres,
                cost=costs, visiting=visits), high


TIMING_SHAPE, TIMING_RES = (98, 98), 0.1


def timing_inputs(n_views):
    """The inputs of the timing (tools/scan_map_time.py runs the device on the same ones): aabb, rows [n,640] float32, yaws [n], w_locs [n,3]."""
    rng = np.random.default_rng(5)
    aabb32 = np.array([-4.9, -0.5, -4.9, 4.9, 2.5, 4.9], np.float32)
    rows = make_depth(rng, n_views, 1, 640, 0.5, 4.0)[:, 0]
    w_locs = np.stack([rng.uniform(-1, 1, n_views), np.full(n_views, 1.2), rng.uniform(-1, 1, n_views)], axis=1)
    return aabb32, rows, rng.uniform(-3, 3, n_views), w_locs


def time_reference(PF, n_views):
    aabb32, rows, yaws, w_locs = timing_inputs(n_views)
    align = align_of(640)
    cost_map, visiting = np.full(TIMING_SHAPE, 0.5), np.zeros(TIMING_SHAPE)
    t0 = time.perf_counter()
    for i in range(n_views):
        d_angles = (align + yaws[i]) % (2 * np.pi)
        grid_loc = np.array((w_locs[i] - aabb32[:3]) // TIMING_RES, dtype=int)
        # where a beam leaves on the low side the reference wraps its cells round: harmless for a timing
        cost_map, vmap = PF.update_cost_map(cost_map=cost_map, depth=rows[i], angle=d_angles, g_loc=grid_loc, w_loc=w_locs[i], aabb=aabb32,
                                            resolution=TIMING_RES)
        visiting += vmap
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="the reference tree (planning/planning_funcs.py and perception/data_proc/depth_to_grid.py)")
    ap.add_argument("--out", default=os.path.join(HERE, "scan_maps.npz"))
    args = ap.parse_args()
    PF, DG = import_reference(args.reference)
    rng = np.random.default_rng(11)
    out = {}
    # x indices come from world x - aabb[2], z indices from world z - aabb[0]: the cameras and depths keep both non-negative
    case, high_small = make_case(PF, DG, rng, (24, 20), 0.2, (-2.0, -1.6), V=5, H=3, W=64, cam_x=(0.4, 1.6), cam_z=(-0.3, 1.0), depth_range=(0.3, 1.6))
    out.update({"small_" + k: v for k, v in case.items()})
    case, high_wide = make_case(PF, DG, rng, (98, 90), 0.1, (-4.9, -4.5), V=3, H=2, W=640, cam_x=(-1.0, 2.0), cam_z=(-1.4, 2.0), depth_range=(0.5, 3.4))
    out.update({"wide_" + k: v for k, v in case.items()})
    assert high_small + high_wide > 0                                                 # a cell skipped on the high side
    np.savez_compressed(args.out, **out)
    print("wrote", args.out, os.path.getsize(args.out), "bytes")
    for n in (6, 39):
        t = min(time_reference(PF, n) for _ in range(3))
        print(f"reference update_cost_map, {n} views of 640 beams on 98 x 98: {t * 1e3:.1f} ms on this host (best of 3)")


if __name__ == "__main__":
    main()
