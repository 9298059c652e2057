"""Measurement of the planner cost map (DESIGN.md "Planner cost map", profiles/scan_map.txt): one `ScanCostMap.update` for the 6 views
of a planning step and the 39 views of the initialisation (scripts/pipeline.py:272-292, :1115-1138), 640 beams each, on a 98 x 98 map,
on the inputs tests/golden/make_golden_scanmap.py times the reference's update_cost_map loop on; then `goal_cells` and `draw_goals` of
20 goals on the resulting map.

  1. Device events around each call, legs interleaved in one loop, warm-ups, medians (min-max).  "update" is the whole Python call with
     the depth images already on the device (the small host copy of yaw, location and centre is inside); "abi" is mnf_scan_map_update
     alone with every input on the device.
  2. The numpy restatement tests/scanmap_ref.py on the host for the same inputs, and whether the device map has the same cells.

    python tools/scan_map_time.py [--reps 21] [--out FILE]
"""
import argparse
import ctypes
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tests", "golden"))
sys.path.insert(0, os.path.join(REPO, "tools"))
import apnrf_amd  # noqa: E402,F401
import scanmap_ref as SR  # noqa: E402
from apnrf_amd import _lib as L  # noqa: E402
from apnrf_amd import planning as PL  # noqa: E402
from make_golden_scanmap import TIMING_RES, TIMING_SHAPE, timing_inputs  # noqa: E402
from object_map_measure import event_ms  # noqa: E402

DEV = "cuda:0"
H = 640


def poses_of(yaws, w_locs):
    p = np.tile(np.eye(4), (len(yaws), 1, 1))
    p[:, 0, 0], p[:, 0, 2], p[:, 2, 0], p[:, 2, 2] = np.cos(yaws), np.sin(yaws), -np.sin(yaws), np.cos(yaws)
    p[:, :3, 3] = w_locs
    return p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("scan_map_time needs a GPU: nothing here is a measurement without one")
    lib = L.load_library()
    legs, notes, keep = {}, [], []
    for n in (6, 39):
        aabb32, rows, yaws, w_locs = timing_inputs(n)
        poses = poses_of(yaws, w_locs)
        depth = np.random.default_rng(1).uniform(0.5, 4.0, (n, H, 640)).astype(np.float32)
        depth[:, H // 2] = rows
        d_depth = torch.from_numpy(depth).to(DEV)
        m = PL.ScanCostMap(aabb32, TIMING_RES, device=DEV)
        assert (m.nx, m.nz) == TIMING_SHAPE
        yaw, loc, centre = m.view_inputs(poses)
        m.update(d_depth, poses)
        codes, visits = np.zeros(TIMING_SHAPE, np.int32), np.zeros(TIMING_SHAPE, np.int32)
        t0 = time.perf_counter()
        info = SR.scan_update(codes, visits, rows, PL.align_angles(640), yaw, loc, centre, aabb32.astype(np.float64), TIMING_RES)
        host_s = time.perf_counter() - t0
        same = np.array_equal(m.codes.cpu().numpy(), codes) and np.array_equal(m.visits.cpu().numpy(), visits)
        differ = int((m.codes.cpu().numpy() != codes).sum())
        notes.append(f"{n} views: restatement on the host {host_s * 1e3:.0f} ms | same cells {same} ({differ} differ; the depths are not moved off "
                     f"half-integers here) | info {m.info()} | restatement {info.tolist()}")
        d_align, d_yaw, d_loc, d_centre = (torch.from_numpy(np.ascontiguousarray(x)).to(DEV) for x in (PL.align_angles(640), yaw, loc, centre))
        box = (ctypes.c_double * 6)(*[float(v) for v in aabb32])
        info_t = torch.zeros(4, dtype=torch.int64, device=DEV)
        keep.append((d_depth, d_align, d_yaw, d_loc, d_centre, box, info_t, m))

        def abi(m=m, d=d_depth, al=d_align, y=d_yaw, lo=d_loc, c=d_centre, box=box, it=info_t, n=n):
            L.launch(lib.mnf_scan_map_update, L.ptr(m.state), m.nx, m.nz, L.ptr(d), n, H, 640, L.ptr(al), L.ptr(y), L.ptr(lo), L.ptr(c), box, TIMING_RES,
                     L.ptr(it))
        legs[f"update{n}"] = (None, lambda m=m, d=d_depth, p=poses: m.update(d, p))
        legs[f"abi{n}"] = (None, abi)
    m = keep[-1][-1]
    blocked = (m.codes == 2).to(torch.int32)
    g = PL.goal_cells(blocked, m.visits)
    u = torch.from_numpy(np.random.default_rng(2).random(20)).to(DEV)
    legs["goal_cells"] = (None, lambda: PL.goal_cells(blocked, m.visits))
    legs["draw_goals"] = (None, lambda: PL.draw_goals(g["cells"], g["count"], u))
    ms = event_ms(legs, a.reps, warmup=3)

    def row(k):
        med, lo, hi = ms[k]
        return f"{med:8.3f} ms ({lo:.3f}-{hi:.3f})"
    lines = [f"# planner cost map: {TIMING_SHAPE[0]} x {TIMING_SHAPE[1]} cells of {TIMING_RES} m, views of 640 beams (depth images 640 x 640 on the device); "
             f"medians of {a.reps} repetitions (min-max), legs interleaved, device events",
             f"ScanCostMap.update, 6 views              {row('update6')} | the whole call: host yaw / centre, one small copy, memset, two launches",
             f"mnf_scan_map_update, 6 views             {row('abi6')} | one workgroup of 1024 threads per view, {TIMING_SHAPE[0] * TIMING_SHAPE[1] * 4} B of LDS each",
             f"ScanCostMap.update, 39 views             {row('update39')}",
             f"mnf_scan_map_update, 39 views            {row('abi39')}",
             f"goal_cells, no field                     {row('goal_cells')} | {int(g['count'].item())} goals listed; the decay table's upload is inside",
             f"draw_goals, 20 goals                     {row('draw_goals')}"] + ["host  " + s for s in notes]
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
