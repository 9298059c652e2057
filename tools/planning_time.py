"""Measurement of the planner grid search (DESIGN.md "Planner grid search", profiles/planning_paths.txt): one planning step's worth on a
98 x 98 rooms map with walls and doors, start in the middle: ONE shortest-path field (`mnf_path_field`) plus ONE trace of 20 goals
(`mnf_path_trace`), which replace the 20 `Dijkstra.planning` calls of sample_traj (planning_funcs.py:288-326).

  1. Device events around each call, legs interleaved in one loop, warm-ups, medians (min-max): the field, the 20-goal trace, a batch of
     20 fields from 20 starts in one launch, the field of the 198 x 198 serpentine (the worst case at the size cap), and the sweeps each ran.
  2. The wall time of `Dijkstra.planning_many` for the 20 goals from a cold cache (field, trace, host copy and the Python lists) and of a
     second call from the same start (trace only).
  3. The numpy restatement tests/planning_ref.py on the host for the same map, and whether the device field has the same labels.

    python tools/planning_time.py [--reps 21] [--out FILE]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tools"))
import apnrf_amd  # noqa: E402,F401
import planning_ref as PR  # noqa: E402
from apnrf_amd import planning as PL  # noqa: E402
from object_map_measure import event_ms  # noqa: E402

DEV = "cuda:0"
RES = 0.2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("planning_time needs a GPU: nothing here is a measurement without one")
    rooms = PR.rooms_map(98, 14)
    start = (49, 49)
    t0 = time.perf_counter()
    want, reached = PR.path_field(rooms, start)
    host_field_s = time.perf_counter() - t0
    rng = np.random.default_rng(0)
    cells = np.argwhere(want != PR.UNREACHED)
    goals = cells[rng.choice(len(cells), 20, replace=False)]
    t0 = time.perf_counter()
    ref_paths, ref_offsets, ref_lengths = PR.trace_many(want[None], np.concatenate([np.zeros((20, 1), np.int64), goals], axis=1))
    host_trace_s = time.perf_counter() - t0

    d_rooms = torch.from_numpy(rooms).to(DEV)
    d_src = torch.tensor([start], dtype=torch.int32, device=DEV)
    d_goals = torch.from_numpy(np.concatenate([np.zeros((20, 1), np.int64), goals], axis=1).astype(np.int32)).to(DEV)
    starts20 = cells[rng.choice(len(cells), 20, replace=False)].astype(np.int32)
    d_src20 = torch.from_numpy(starts20).to(DEV)
    serp = torch.from_numpy(PR.serpentine(198)).to(DEV)
    d_zero = torch.zeros(1, 2, dtype=torch.int32, device=DEV)
    out = PL.path_field(d_rooms, d_src)
    same_field = np.array_equal(out["field"][0].cpu().numpy().view(np.uint32), want)
    t = PL.trace_paths(out["field"], d_goals)
    same_paths = np.array_equal(t["paths"].cpu().numpy(), ref_paths) and np.array_equal(t["offsets"].cpu().numpy(), ref_offsets)
    sweeps = {"rooms": int(out["info"][0, 1]), "rooms20": PL.path_field(d_rooms, d_src20)["info"][:, 1].cpu().numpy(),
              "serpentine": int(PL.path_field(serp, d_zero)["info"][0, 1])}
    field = out["field"]
    legs = {"field": (None, lambda: PL.path_field(d_rooms, d_src)),
            "trace": (None, lambda: PL.trace_paths(field, d_goals)),                   # holds the one host read of the total
            "fields20": (None, lambda: PL.path_field(d_rooms, d_src20)),
            "serpentine": (None, lambda: PL.path_field(serp, d_zero))}
    ms = event_ms(legs, a.reps, warmup=3)

    goals_xy = [(float(x) * RES, float(y) * RES) for x, y in goals]
    cold, warm = [], []
    for _ in range(a.reps):
        d = PL.Dijkstra([0.0, 0.0, 0.0, 98 * RES, 98 * RES, 1.0], d_rooms, RES, 0.05, device=DEV)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = d.planning_many(start[0] * RES, start[1] * RES, goals_xy)
        cold.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        d.planning_many(start[0] * RES, start[1] * RES, goals_xy)
        warm.append(time.perf_counter() - t0)
    assert all(g is not None for g in got) and [len(g[0]) for g in got] == ref_lengths.tolist()

    def row(k):
        m, lo, hi = ms[k]
        return f"{m:8.3f} ms ({lo:.3f}-{hi:.3f})"
    lines = [
        f"# planner grid search: 98 x 98 rooms map (walls every 14 cells, a door per wall segment, one closed room), start {start}, {reached} cells reached; "
        f"medians of {a.reps} repetitions (min-max), legs interleaved, device events",
        f"mnf_path_field, one source               {row('field')} | {sweeps['rooms']} sweeps, one workgroup of 1024 threads, {100 * 100 * 4} B of LDS",
        f"mnf_path_trace, 20 goals (+ torch glue)  {row('trace')} | {int(ref_lengths.sum())} cells written; the gather, cumsum and one host read of the total are inside",
        f"mnf_path_field, 20 sources, one launch   {row('fields20')} | sweeps {int(sweeps['rooms20'].min())}-{int(sweeps['rooms20'].max())}",
        f"mnf_path_field, 198 x 198 serpentine     {row('serpentine')} | {sweeps['serpentine']} sweeps for a longest way of 19503 moves: the worst case at the size cap",
        f"wall  Dijkstra.planning_many, 20 goals, cold cache (field + trace + host copy + Python lists): {np.median(cold) * 1e3:.3f} ms "
        f"({np.min(cold) * 1e3:.3f}-{np.max(cold) * 1e3:.3f}); same start again (trace only): {np.median(warm) * 1e3:.3f} ms",
        f"host  tests/planning_ref.py (heapq, exact integer order) on this machine's CPU, once ({os.cpu_count()} CPUs, numpy {np.__version__}): "
        f"field {host_field_s * 1e3:.0f} ms, 20 traces {host_trace_s * 1e3:.1f} ms | same labels {same_field}, same paths {same_paths}",
    ]
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
