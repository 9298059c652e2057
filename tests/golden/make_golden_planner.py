"""Writes tests/golden/planner_paths.npz: what the reference's own `Dijkstra.planning` (planning/dijkstra.py) returns on small maps.

    python tests/golden/make_golden_planner.py --reference /path/to/the/reference/tree

The reference class is imported at generation time only; the fixture holds data: the maps, resolution and aabb, the start, and per goal
the reference's None flag and the (a, b) make-up (straight, diagonal steps) and length of the path it returned.  Runs on the CPU, about
20 s.  The generator asserts, on the reference's answers alone, that the fixture holds the cases the tests rely on."""
import argparse
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import planning_ref as PR  # noqa: E402  (the map builders only)

RES = 0.2
SMALL_SEED = 3
RING = (14, 21, 3, 10)               # x0, x1, y0, y1 of a closed 4-connected wall on the small map


def small_map():
    m = PR.seeded_map((24, 20), SMALL_SEED, 0.3)
    x0, x1, y0, y1 = RING
    m[x0, y0:y1 + 1] = 1
    m[x1, y0:y1 + 1] = 1
    m[x0:x1 + 1, y0] = 1
    m[x0:x1 + 1, y1] = 1
    return m


def run_case(Dijkstra, grid, aabb, start_cell, goal_cells):
    d = Dijkstra(aabb, grid, RES, 0.05)
    sx, sy = start_cell[0] * RES, start_cell[1] * RES
    assert (d.calc_xy_index(sx, 0), d.calc_xy_index(sy, 0)) == tuple(start_cell)
    goals = np.array([[gx * RES, gy * RES] for gx, gy in goal_cells], np.float64)
    none, ab, length, squeezes = [], [], [], 0
    for (gx, gy), (wx, wy) in zip(goal_cells, goals):
        assert (d.calc_xy_index(wx, 0), d.calc_xy_index(wy, 0)) == (gx, gy)
        r = d.planning(sx, sy, wx, wy)
        if r is None:
            none.append(True); ab.append((0, 0)); length.append(0)
            continue
        cells = np.array([[round(x / RES), round(y / RES)] for x, y in zip(*r)], np.int64)
        assert tuple(cells[0]) == (gx, gy) and tuple(cells[-1]) == tuple(start_cell)
        none.append(False); ab.append(PR.make_up(cells)); length.append(len(cells))
        for p, q in zip(cells[:-1], cells[1:]):
            if abs(p - q).sum() == 2 and grid[p[0], q[1]] and grid[q[0], p[1]]:
                squeezes += 1
    return dict(map=grid.astype(np.int32), aabb=np.asarray(aabb, np.float64), res=np.float64(RES), start=np.array([sx, sy], np.float64),
                start_cell=np.array(start_cell, np.int32), goals=goals, goal_cells=np.array(goal_cells, np.int32).reshape(-1, 2),
                none=np.array(none, bool), ab=np.array(ab, np.int32).reshape(-1, 2), len=np.array(length, np.int32)), squeezes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="the reference tree (its planning/dijkstra.py is imported)")
    ap.add_argument("--out", default=os.path.join(HERE, "planner_paths.npz"))
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(args.reference, "planning"))
    from dijkstra import Dijkstra
    t0 = time.time()
    out = {}

    grid = small_map()
    nx, ny = grid.shape
    aabb = [-1.0, -2.0, 0.0, -1.0 + nx * RES, -2.0 + ny * RES, 1.0]
    start = (3, 4)
    assert grid[start] == 0
    every = [(x, y) for x in range(nx) for y in range(ny)]
    # all 480 cells, then two goals whose rounded index falls outside the map
    case, squeezes = run_case(Dijkstra, grid, aabb, start, every + [(nx, 5), (-1, 3)])
    none = case["none"][:nx * ny].reshape(nx, ny)
    free = grid == 0
    assert PR.limits_of(aabb, grid.shape, RES) == (nx, ny)
    assert none[grid != 0].all()                                                   # no blocked goal is ever reached
    unreached_free = (none & free).sum()
    x0, x1, y0, y1 = RING
    assert (none | ~free)[x0 + 1:x1, y0 + 1:y1].all() and free[x0 + 1:x1, y0 + 1:y1].sum() > 10      # the pocket behind the 4-connected wall
    assert unreached_free >= 0.05 * free.sum(), (unreached_free, free.sum())
    assert (~none).sum() >= 0.25 * free.sum()
    assert squeezes > 0                                                            # a diagonal step between two obstacles touching at a corner
    assert not case["none"][every.index(start)] and case["len"][every.index(start)] == 1              # the goal equal to the start
    assert case["none"][-2:].all()                                                 # goals outside the map
    out.update({"small_" + k: v for k, v in case.items()})
    print(f"small: {free.sum()} free, {unreached_free} of them unreached, {squeezes} squeezed steps ({time.time() - t0:.1f} s)")

    # the same map under an aabb whose max_x cuts off the last two x indices
    cut = [-1.0, -2.0, 0.0, -1.0 + (nx - 2) * RES, -2.0 + ny * RES, 1.0]
    assert PR.limits_of(cut, grid.shape, RES) == (nx - 2, ny)
    case, _ = run_case(Dijkstra, grid, cut, start, every)
    none_cut = case["none"].reshape(nx, ny)
    assert none_cut[nx - 2:].all() and free[nx - 2:].any() and not none[nx - 2:][free[nx - 2:]].all()
    out.update({"cut_" + k: v for k, v in case.items()})

    # a blocked start cell
    bstart = tuple(int(v) for v in np.argwhere(grid[:10, :10] != 0)[7])
    assert grid[bstart] != 0
    case, _ = run_case(Dijkstra, grid, aabb, bstart, every[::8] + [bstart])
    assert not case["none"][-1] and case["len"][-1] == 1 and (~case["none"]).sum() > 10
    out.update({"blocked_start_" + k: v for k, v in case.items()})
    print(f"cut and blocked start done ({time.time() - t0:.1f} s)")

    rooms = PR.rooms_map(98, 14)
    raabb = [0.0, 0.0, 0.0, 98 * RES, 98 * RES, 1.0]
    rstart = (49, 49)
    assert rooms[rstart] == 0
    rng = np.random.default_rng(7)
    cells = np.argwhere(rooms == 0)
    picks = [tuple(int(v) for v in cells[i]) for i in rng.choice(len(cells), 30, replace=False)]
    picks += [(3, 3), (10, 12), (0, 0), (13, 13)]                                  # inside the closed corner room
    picks += [(14, 40), (56, 56), (97, 97), (0, 97), (97, 0), rstart]              # walls, corners, the start
    assert len(picks) == 40
    case, _ = run_case(Dijkstra, rooms, raabb, rstart, picks)
    assert case["none"][30:34].all() and case["none"][34:36].all() and not case["none"][36:].any() and (~case["none"][:30]).sum() > 20
    out.update({"rooms_" + k: v for k, v in case.items()})
    print(f"rooms: {int((~case['none']).sum())} of 40 goals reached, longest path {int(case['len'].max())} cells ({time.time() - t0:.1f} s)")

    np.savez_compressed(args.out, **out)
    print("wrote", args.out, os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    main()
