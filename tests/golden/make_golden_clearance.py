"""Writes tests/golden/clearance_walks.npz: the reference's own voxel lists (planning/planning_funcs.py:97-159,
get_voxels_between_points), its collision_checker answers (:162-179) and its world2voxels (:187-189) on pinned values.

    python tests/golden/make_golden_clearance.py --reference /path/to/the/reference/tree

The reference module is imported at generation time only (what it imports and this container lacks is placeholdered, as
make_golden_scanmap.py does).  The fixture holds data: chords (start, end, the two voxels the reference derives for them, the aabb origin
they were derived with), the listed voxels packed at offsets, the checker's bools on a small two-member grid, and the pinned values with
the reference's indices.  Every chord is driven the way collision_checker drives the walk: positions in world coordinates, voxels from
world2voxels(x - aabb[:3]); with a non-zero aabb origin that mixes two frames, which is the reference's and is kept.  The generator
asserts, on the reference's answers alone, that the fixture holds each kind of case the tests rely on."""
import argparse
import contextlib
import io
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

SIZE = 0.2
SHAPE = (12, 10, 8)
ORIGIN = np.array([-0.6, 0.4, -0.2])
KINDS = ("octant", "axis", "zero", "same_voxel", "faces", "leaving", "frames")


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
                 "rotorpy.trajectories.minsnap", "rotorpy.simulate", "tqdm", "matplotlib", "matplotlib.pyplot", "scipy", "scipy.signal",
                 "scipy.spatial.transform"):
        _placeholder(name)
    import planning_funcs
    return planning_funcs


def make_grid(rng):
    g = np.zeros((2,) + SHAPE, np.uint8)
    g[0, 5:7, 2:8, 0:5] = 1                                       # a wall across the middle, open above
    g[0, 10, 8, 6] = 1
    g[0, 0, 0, 0] = 1                                             # a corner voxel: what a walk that left the grid is clipped onto
    g[1] = (rng.uniform(size=SHAPE) < 0.05).astype(np.uint8)      # member 1: never read by the checker
    return g


def make_chords(rng):
    """-> (start [n,3], end [n,3], origin [n,3], kind [n]) in world coordinates."""
    ext = np.array(SHAPE) * SIZE
    rows = []

    def add(kind, s, e, origin):
        rows.append((np.asarray(s, np.float64), np.asarray(e, np.float64), np.asarray(origin, np.float64), KINDS.index(kind)))

    zero = np.zeros(3)
    for octant in range(8):
        sign = np.array([1 if octant >> k & 1 else -1 for k in range(3)], np.float64)
        for _ in range(10):
            s = rng.uniform(0.3 * ext, 0.7 * ext)
            add("octant", s, s + sign * rng.uniform(0.05, 0.28, 3) * ext, zero)
        for _ in range(6):
            s = ORIGIN + rng.uniform(0.3 * ext, 0.7 * ext)
            add("frames", s, s + sign * rng.uniform(0.05, 0.28, 3) * ext, ORIGIN)
    for axis in range(3):
        for sgn in (1.0, -1.0):
            for _ in range(4):
                s = rng.uniform(0.3 * ext, 0.7 * ext)
                e = s.copy()
                e[axis] += sgn * rng.uniform(0.1, 0.29) * ext[axis]
                add("axis", s, e, zero)
    for _ in range(4):
        s = rng.uniform(0.1 * ext, 0.9 * ext)
        add("zero", s, s, zero)
    add("zero", ORIGIN + 0.5 * ext, ORIGIN + 0.5 * ext, ORIGIN)
    add("zero", [0.4, 0.6, 0.2], [0.4, 0.6, 0.2], zero)           # on three faces at once
    for _ in range(10):
        v = rng.integers(1, np.array(SHAPE) - 1)
        add("same_voxel", (v + rng.uniform(0.1, 0.9, 3)) * SIZE, (v + rng.uniform(0.1, 0.9, 3)) * SIZE, zero)
    for _ in range(16):
        a, b = rng.integers(1, np.array(SHAPE) - 1), rng.integers(1, np.array(SHAPE) - 1)
        s, e = a * SIZE, b * SIZE                                 # every coordinate k * 0.2 as float64 forms it
        if rng.uniform() < 0.5:
            e = e + rng.uniform(0.0, 0.19, 3) * (rng.uniform(size=3) < 0.5)
        add("faces", s, e, zero)
    add("leaving", [0.9, 0.5, 0.1], [0.1, 0.1, 0.1], zero)
    add("leaving", [0.3, 0.3, 0.3], [0.05, 0.05, 0.05], zero)
    add("leaving", ext - 0.3, ext - 0.01, zero)
    add("leaving", [1.0, 1.0, 1.5], [1.3, 1.1, 1.59], zero)
    for _ in range(8):
        s = rng.uniform(0.2 * ext, 0.8 * ext)
        e = np.where(rng.uniform(size=3) < 0.5, rng.uniform(0.0, 0.1, 3), ext - rng.uniform(0.0, 0.1, 3))
        add("leaving", s, e, zero)
    return tuple(np.array([r[k] for r in rows]) for k in range(4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="the reference tree (planning/planning_funcs.py)")
    ap.add_argument("--out", default=os.path.join(HERE, "clearance_walks.npz"))
    args = ap.parse_args()
    PF = import_reference(args.reference)
    rng = np.random.default_rng(23)
    grid = make_grid(rng)
    start, end, origin, kind = make_chords(rng)
    n = start.shape[0]
    cur = np.empty((n, 3), np.int64)
    endv = np.empty((n, 3), np.int64)
    lists, checker = [], np.zeros(n, bool)
    for i in range(n):
        aabb = np.concatenate([origin[i], origin[i] + np.array(SHAPE) * SIZE])
        x = np.stack([start[i], 0.5 * (start[i] + end[i]), end[i]])
        idx = PF.world2voxels(x - aabb[:3], SIZE)
        cur[i], endv[i] = idx[0], idx[-1]
        lists.append(np.array(PF.get_voxels_between_points(x[0], x[-1], idx[0], idx[-1], SIZE), np.int64).reshape(-1, 3))
        with contextlib.redirect_stdout(io.StringIO()):
            checker[i] = bool(PF.collision_checker(grid, {"x": x}, SIZE, aabb))
    offsets = np.zeros(n + 1, np.int64)
    offsets[1:] = np.cumsum([v.shape[0] for v in lists])
    voxels = np.concatenate(lists)
    pinned = np.array([k * 0.2 for k in range(41)] + [1.2000000000000002, -1e-17, -0.2])
    pinned_cells = np.asarray(PF.world2voxels(pinned, SIZE), np.int64)

    # the fixture's conditions, on the reference's answers alone
    shape = np.array(SHAPE)
    for k, name in enumerate(KINDS):
        assert (kind == k).sum() >= 6, name
    assert 180 <= n <= 260, n
    signs = {tuple(np.sign(end[i] - start[i]).astype(int)) for i in range(n) if kind[i] == KINDS.index("octant")}
    assert len(signs) == 8
    for i in range(n):
        v = lists[i]
        assert v.shape[0] >= 1 and not (v == cur[i]).all(axis=1).any(), i             # the start voxel is never listed
        if kind[i] == KINDS.index("zero"):
            assert v.tolist() == [(cur[i] + [0, 0, 1]).tolist()], i                   # one step in +z
        if kind[i] == KINDS.index("same_voxel"):
            assert (cur[i] == endv[i]).all() and v.shape[0] == 1, i
    first_leaving = int(np.argmax(kind == KINDS.index("leaving")))
    assert lists[first_leaving][-1].tolist() == [-1, 0, 0]
    outside = [((v < 0) | (v >= shape)).any() for v in lists]
    assert sum(outside) >= 8
    assert (np.abs(voxels).max() < 1000) and max(v.shape[0] for v in lists) < 400
    assert checker.any() and (~checker).any()
    assert checker[kind == KINDS.index("frames")].any() and (~checker[kind == KINDS.index("frames")]).any()
    differ = pinned_cells != np.floor(pinned / SIZE).astype(np.int64)
    assert differ.any() and pinned_cells[5] == 4 and pinned_cells[-2] == -1 and pinned_cells[-1] in (-1, -2)
    on_face = [(np.abs(start[i] / SIZE - np.rint(start[i] / SIZE)) < 1e-9).all() for i in range(n)]
    assert sum(on_face) >= 16
    print(f"{n} chords, {voxels.shape[0]} listed voxels, {sum(outside)} walks leave the grid, {int(checker.sum())} collide, "
          f"{int(differ.sum())} pinned values where // differs from floor(x / size)")
    np.savez_compressed(args.out, size=np.float64(SIZE), shape=shape.astype(np.int32), grid=grid, start=start, end=end, origin=origin,
                        kind=kind.astype(np.int32), kinds=np.array(KINDS), current_voxel=cur.astype(np.int32), end_voxel=endv.astype(np.int32),
                        voxels=voxels.astype(np.int32), offsets=offsets, checker=checker, pinned=pinned, pinned_cells=pinned_cells)
    size = os.path.getsize(args.out)
    assert size < 200 * 1024, size
    print("wrote", args.out, size, "bytes")


if __name__ == "__main__":
    main()
