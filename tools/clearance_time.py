"""Measurement of the trajectory-clearance unit (DESIGN.md "Trajectory clearance", profiles/clearance.txt).

  field   `mnf_clearance_field` on two members at the yaml's grid (aabb of scripts/config_102344250.yaml at main_grid_size 0.2: 98 x 17 x 98),
          at 128^3 and at 256^3: device events, medians (min-max) after warm-ups.  Beside it the host route on the same grid: the copy of the
          members' grids to the host and `scipy.ndimage.distance_transform_edt` of their union (where scipy imports), and whether the two agree.
  lookup  20 trajectories x 400 samples on the yaml's grid: `mnf_clearance_lookup` and `trajectory_clearance` with its torch values (device
          events around each call), and numpy's floor division and gather on the host for the same samples.
  sweep   the voxel walk of the 20 x 399 segments: `ClearanceField.sweep` (device events, one walk launch) against the reference-style Python walk
          (tests/clearance_ref.py, which restates planning_funcs.py:97-159) on the host, once.

Every GPU step is a child process of its own under `timeout`; the driver starts no GPU work itself, stops at the first step that fails and
writes what the steps printed.

    python tools/clearance_time.py [--reps 15] [--out profiles/clearance.txt]
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
VOXEL = 0.2
YAML_AABB = np.array([-19.1, -0.2, -19.1, 0.5, 3.2, 0.5])
STEPS = (("field_yaml", 120), ("field_128", 120), ("field_256", 240), ("lookup", 120), ("sweep", 240))


def rooms_grid(shape, seed, members=2):
    """A floor, walls every 14 voxels with door openings, and clutter; the members differ in the clutter."""
    X, Y, Z = shape
    rng = np.random.default_rng(seed)
    g = np.zeros((members, X, Y, Z), np.uint8)
    g[:, :, 0, :] = 1
    for k in range(14, max(X, Z), 14):
        if k < X:
            g[:, k, :, :] = 1
            for d in range(5, Z - 4, 14):
                g[:, k, 1:min(Y, 11), d:d + 4] = 0
        if k < Z:
            g[:, :, :, k] = 1
            for d in range(5, X - 4, 14):
                g[:, d:d + 4, 1:min(Y, 11), k] = 0
    for m in range(members):
        g[m] |= (rng.uniform(size=shape) < 0.002).astype(np.uint8)
    return g


def yaml_shape():
    return tuple(int(v) for v in np.rint((YAML_AABB[3:] - YAML_AABB[:3]) / VOXEL))


def trajectories(shape, n_traj=20, n_samples=400, seed=3):
    """Smooth random flights inside the box, 5 cm between samples on average."""
    rng = np.random.default_rng(seed)
    ext = np.array(shape) * VOXEL
    out = []
    for _ in range(n_traj):
        p = YAML_AABB[:3] + rng.uniform(0.2, 0.8, 3) * ext
        v = rng.normal(size=3) * [1.0, 0.15, 1.0]
        pts = []
        for _ in range(n_samples):
            v = v + rng.normal(size=3) * [0.2, 0.03, 0.2]
            v *= 0.05 / np.linalg.norm(v)
            p = np.clip(p + v, YAML_AABB[:3] + 0.05, YAML_AABB[:3] + ext - 0.05)
            pts.append(p.copy())
        out.append(np.array(pts))
    pts = np.concatenate(out)
    return pts, np.arange(n_traj + 1, dtype=np.int64) * n_samples


def fmt(t):
    return f"{t[0]:9.3f} ms ({t[1]:.3f}-{t[2]:.3f})"


def step_field(name, reps):
    import torch
    from apnrf_amd import clearance as C
    from object_map_measure import event_ms
    shape = {"field_yaml": yaml_shape(), "field_128": (128, 128, 128), "field_256": (256, 256, 256)}[name]
    g = rooms_grid(shape, 1)
    aabb = np.concatenate([YAML_AABB[:3], YAML_AABB[:3] + np.array(shape) * VOXEL])
    d_g = torch.from_numpy(g).to(DEV)
    f = C.clearance_field(d_g, aabb=aabb, voxel=VOXEL)
    ms = event_ms({"field": (None, lambda: C.clearance_field(d_g, aabb=aabb, voxel=VOXEL))}, reps, warmup=3)
    info = f.info.cpu().tolist()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    host = d_g.cpu().numpy()
    copy_s = time.perf_counter() - t0
    line = (f"{name:10s} {shape[0]} x {shape[1]} x {shape[2]}, 2 members, {info[0]} occupied, largest d2 {info[1]}: mnf_clearance_field {fmt(ms['field'])}"
            f" = {np.prod(shape) / ms['field'][0] * 1e-6:.2f} G voxels/s")
    try:
        from scipy import ndimage
    except ImportError:
        print(line + f" | host: copy of the grids {copy_s * 1e3:.2f} ms; scipy is not installed, no host transform was timed")
        return
    t0 = time.perf_counter()
    edt = ndimage.distance_transform_edt(~(host != 0).any(axis=0))
    edt_s = time.perf_counter() - t0
    same = np.array_equal(np.rint(edt * edt).astype(np.int64), f.d2.cpu().numpy().astype(np.int64))
    print(line + f" | host: copy of the grids {copy_s * 1e3:.2f} ms + scipy.ndimage.distance_transform_edt of the union {edt_s * 1e3:.1f} ms (once, "
          f"scipy {__import__('scipy').__version__}); squared, the same integers: {same}")
    if not same:
        raise SystemExit(1)


def step_lookup(reps):
    import torch
    from apnrf_amd import clearance as C
    from object_map_measure import event_ms
    shape = yaml_shape()
    aabb = np.concatenate([YAML_AABB[:3], YAML_AABB[:3] + np.array(shape) * VOXEL])
    f = C.clearance_field(torch.from_numpy(rooms_grid(shape, 1)).to(DEV), aabb=aabb, voxel=VOXEL)
    pts, offsets = trajectories(shape)
    d_p, d_o = torch.from_numpy(pts).to(DEV), torch.from_numpy(offsets).to(DEV)
    ms = event_ms({"lookup": (None, lambda: f.lookup(d_p, d_o)), "values": (None, lambda: f.trajectory_clearance(d_p, d_o, radius=0.1))}, reps, warmup=3)
    out = f.trajectory_clearance(d_p, d_o, radius=0.1, host=True)
    d2 = f.d2.cpu().numpy()
    host = []
    for _ in range(reps):
        t0 = time.perf_counter()
        cells = np.array((pts - aabb[:3]) // VOXEL, dtype=int)
        v = d2[cells[:, 0], cells[:, 1], cells[:, 2]].reshape(20, 400)
        least, first = v.min(axis=1), v.argmin(axis=1)
        host.append(time.perf_counter() - t0)
    same = np.array_equal(out["summary"]["traj"][:, 0], least) and np.array_equal(out["summary"]["traj"][:, 1], first)
    print(f"lookup     20 trajectories x 400 samples on {shape[0]} x {shape[1]} x {shape[2]}: mnf_clearance_lookup (+ torch glue) {fmt(ms['lookup'])}; "
          f"trajectory_clearance with metres, lower, margin, certified {fmt(ms['values'])}; {int(out['summary']['certified'].sum())} of 20 certified at 0.1 m"
          f" | host: numpy // and gather on the copied field {np.median(host) * 1e3:.3f} ms; same least d2 and first sample: {same}")
    if not same:
        raise SystemExit(1)


def step_sweep(reps):
    import torch
    import clearance_ref as CR
    from apnrf_amd import clearance as C
    from object_map_measure import event_ms
    shape = yaml_shape()
    aabb = np.concatenate([YAML_AABB[:3], YAML_AABB[:3] + np.array(shape) * VOXEL])
    g = rooms_grid(shape, 1)
    f = C.clearance_field(torch.from_numpy(g).to(DEV), aabb=aabb, voxel=VOXEL)
    pts, offsets = trajectories(shape)
    d_p, d_o = torch.from_numpy(pts).to(DEV), torch.from_numpy(offsets).to(DEV)
    ms = event_ms({"sweep": (None, lambda: f.sweep(d_p, d_o))}, reps, warmup=3)
    hits = f.sweep(d_p, d_o)["hits"].cpu().numpy()
    rel = pts - aabb[:3]
    t0 = time.perf_counter()
    cells = np.array(rel // VOXEL, dtype=int)
    union = (g != 0).any(axis=0)
    want = np.full_like(hits, -1)
    want[:, 4] = 0
    for t in range(20):
        for i in range(offsets[t], offsets[t + 1] - 1):
            want[i] = CR.walk_hit(CR.voxel_walk(rel[i], rel[i + 1], cells[i], cells[i + 1], VOXEL)[0], union)
    host_s = time.perf_counter() - t0
    same = np.array_equal(hits, want)
    print(f"sweep      the voxel walks of 20 x 399 segments against both members ({int(hits[:, 4].sum())} voxels, {int((hits[:, 0] >= 0).sum())} segments meet a voxel): "
          f"ClearanceField.sweep (lookup + mnf_voxel_walk_hits + torch glue) {fmt(ms['sweep'])} | host: the reference-style Python walk with the clipped look-up "
          f"(tests/clearance_ref.py) {host_s:.2f} s, once; same rows: {same}")
    if not same:
        raise SystemExit(1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", default=None, help="(internal) run one GPU step in this process")
    a = ap.parse_args()
    if a.step:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("clearance_time needs a GPU: nothing here is a measurement without one")
        import apnrf_amd  # noqa: F401
        if a.step.startswith("field"):
            step_field(a.step, a.reps)
        else:
            {"lookup": step_lookup, "sweep": step_sweep}[a.step](a.reps)
        return
    lines = [f"# trajectory clearance; medians of {a.reps} repetitions (min-max) after 3 warm-ups, device events around each call; the host figures are "
             f"this machine's CPU ({os.cpu_count()} CPUs, numpy {np.__version__}).  No speed bar was set beforehand: these are the first measurements of either side."]
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
