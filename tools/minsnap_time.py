"""Measurement of the min-snap trajectory unit (DESIGN.md "Min-snap candidate trajectories", profiles/minsnap.txt).

For paths of 40, 80 and 150 waypoints (random 8-connected walks at 0.2 m, as the grid search lists them), 20 and 256 trajectories a call:
  solve   `trajectory.min_snap_cells` (one `mnf_minsnap_solve` launch);
  sample  `MinSnapCurves.sample` (count, the one host read of the totals, fill);
device events around each call, the two batch sizes and the two calls interleaved in every repetition, medians (min-max) after warm-ups.
Beside them, timed once per trajectory on this machine's host for three of the paths: the restatement's `dense=True` route
(tests/minsnap_ref.py: four SVD rank tests and four dense solves of the 8 m x 8 m system, the reference's arithmetic; the reference itself
is not needed) and its banded route.

Every GPU step is a child process of its own under `timeout`; the driver starts no GPU work itself, stops at the first step that fails and
writes what the steps printed.

    python tools/minsnap_time.py [--reps 15] [--out profiles/minsnap.txt]
"""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tools"))

DEV = "cuda:0"
STEPS = (("40", 180), ("80", 180), ("150", 240))
MOVES = [(1, 0), (0, 1), (-1, 0), (0, -1), (-1, -1), (-1, 1), (1, -1), (1, 1)]


def walks(n_traj, n_waypoints, seed):
    """[n_traj * n_waypoints, 2] int32 cells and their offsets; a walk never repeats the cell it stands on."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n_traj):
        c = [(int(rng.integers(100, 200)), int(rng.integers(100, 200)))]
        move = MOVES[int(rng.integers(8))]
        while len(c) < n_waypoints:
            if rng.uniform() > 0.7:
                move = MOVES[int(rng.integers(8))]
            c.append((c[-1][0] + move[0], c[-1][1] + move[1]))
        out.append(np.array(c, np.int32))
    return np.concatenate(out), np.arange(n_traj + 1, dtype=np.int64) * n_waypoints


def fmt(t):
    return f"{t[0]:8.3f} ms ({t[1]:.3f}-{t[2]:.3f})"


def step(n_waypoints, reps):
    import torch
    import minsnap_ref as MR
    from apnrf_amd import trajectory as TJ
    from object_map_measure import event_ms
    origin = np.array([-19.1, -0.2, -19.1])
    legs, curves, info = {}, {}, {}
    for T in (20, 256):
        cells, offsets = walks(T, n_waypoints, 7 + T)
        d_c, d_o = torch.from_numpy(cells).to(DEV), torch.from_numpy(offsets).to(DEV)
        curves[T] = TJ.min_snap_cells(d_c, d_o, 0.2, origin)
        out = curves[T].sample()
        status = curves[T].status.cpu().numpy()
        info[T] = (int((status == TJ.OK).sum()), int(out["times"].shape[0]), cells, offsets)
        legs[f"solve{T}"] = (None, lambda d_c=d_c, d_o=d_o: TJ.min_snap_cells(d_c, d_o, 0.2, origin))
        legs[f"sample{T}"] = (None, lambda T=T: curves[T].sample())
    ms = event_ms(legs, reps, warmup=3)
    host = {"dense": [], "banded": []}
    cells, offsets = info[20][2], info[20][3]
    for k in range(3):
        pts = MR.waypoints_of_cells(cells[offsets[k]:offsets[k + 1]], 0.2, origin)
        for route in ("dense", "banded"):
            t0 = time.perf_counter()
            r = MR.restate(pts, dense=route == "dense")
            host[route].append(time.perf_counter() - t0)
            assert r["status"] == MR.OK
    parts = [f"{n_waypoints:3d} waypoints:"]
    for T in (20, 256):
        parts.append(f"{T} trajectories ({info[T][0]} accepted, {info[T][1]} samples) solve {fmt(ms[f'solve{T}'])} sample {fmt(ms[f'sample{T}'])};")
    parts.append(f"host, per trajectory, median of 3: restatement dense=True (solve + sample) {np.median(host['dense']) * 1e3:.0f} ms, banded "
                 f"{np.median(host['banded']) * 1e3:.0f} ms")
    print(" ".join(parts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", default=None, help="(internal) run one GPU step in this process")
    a = ap.parse_args()
    if a.step:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("minsnap_time needs a GPU: nothing here is a measurement without one")
        import apnrf_amd  # noqa: F401
        step(int(a.step), a.reps)
        return
    lines = [f"# min-snap candidate trajectories; medians of {a.reps} repetitions (min-max) after 3 warm-ups, device events around each call, batch sizes and "
             f"calls interleaved; the host figures are this machine's CPU ({os.cpu_count()} CPUs, numpy {np.__version__}).  No speed bar was set."]
    failed = None
    for name, limit in STEPS:
        r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", name, "--reps", str(a.reps)],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        body = [ln for ln in r.stdout.splitlines() if ln.strip() and "amdgpu.ids" not in ln]
        if r.returncode != 0:
            failed = f"# step {name} ended with status {r.returncode}; nothing further was started\n" + "\n".join(body[-12:])
            break
        lines += body[-1:]
        print(body[-1] if body else "", flush=True)
    text = "\n".join(lines + ([failed] if failed else []))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    if failed:
        print(failed)
        raise SystemExit(1)


if __name__ == "__main__":
    main()
