"""Measurement of the surface mesh (DESIGN.md "Surface mesh", profiles/surface_mesh.txt), with the library's own profile labels (hipEvent pairs
around each entry point's launches, `mnf_profile_begin/end/query`):

  1. `mnf_surface_extract` on a 513^3 ball lattice (values = r - |p - c|, iso 0), against the time the lattice's 4 (X+1)(Y+1)(Z+1) bytes take at
     the copy bandwidth of the microarchitecture guide, 6.29 TB/s; beside it the same call with capacities 0 (the count pass, the two scans and an
     emit pass that writes nothing), which splits the dense per-point work from the per-vertex and per-triangle work.
  2. The lattice fill of the trained stand-in of scene 102344250 at refine 4: `surface_lattice_points`, `field_density`, `surface_lattice_scatter`.
  3. The wall time of `extract_surface` on that model (host clock around a call that ends in a host copy), iso = occ_thre / render_step_size.

    python tools/surface_measure.py [--n 513] [--refine 4] [--reps 9] [--out FILE] [--extract-only]

`--extract-only` stops after part 1: the form to run under `rocprofv3 --kernel-trace --stats` for the per-kernel split.
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
import apnrf_amd  # noqa: E402,F401
from apnrf_amd import _lib as L  # noqa: E402
from apnrf_amd import scenes as SC  # noqa: E402
from apnrf_amd import standin as ST  # noqa: E402
from apnrf_amd import surface as SF  # noqa: E402

DEV = "cuda:0"
COPY_BW = 6.29e12          # bytes/s: the device-to-device copy the microarchitecture guide measured


def profiled(lib, fn, reps, labels, warmup=2):
    """-> label -> (ms per call, launches per call) from the library's event pairs over `reps` calls of fn."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    L.check(lib.mnf_profile_begin())
    for _ in range(reps):
        fn()
    L.check(lib.mnf_profile_end(None, None))
    out = {}
    for label in labels:
        ms, n = ctypes.c_double(0), ctypes.c_int64(0)
        L.check(lib.mnf_profile_query(label.encode(), ctypes.byref(ms), ctypes.byref(n)))
        out[label] = (ms.value / reps, n.value / reps)
    return out


def ball_lattice(n, radius_frac=0.36):
    ax = torch.arange(n, dtype=torch.float32, device=DEV) - ((n - 1) / 2.0 + 0.13)
    r2 = ax[:, None, None] ** 2 + ax[None, :, None] ** 2 + ax[None, None, :] ** 2
    return (radius_frac * n - r2.sqrt()).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=513)
    ap.add_argument("--refine", type=int, default=4)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=None)
    ap.add_argument("--extract-only", action="store_true", help="part 1 alone (for a kernel trace)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("surface_measure needs a GPU: nothing here is a measurement without one")
    lib = apnrf_amd.load_library()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    # ---- 1. extraction of a ball lattice
    n = a.n
    values = ball_lattice(n)
    cells = (n - 1,) * 3
    o, s = (ctypes.c_float * 3)(0, 0, 0), (ctypes.c_float * 3)(1, 1, 1)
    nbytes = int(lib.mnf_surface_extract_workspace_bytes(*cells))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    info = torch.empty(4, dtype=torch.int64, device=DEV)

    def call(mv, mt, pos, nrm, tri):
        L.launch(lib.mnf_surface_extract, L.ptr(values), *cells, 0.0, o, s, mv, mt, L.ptr(pos), L.ptr(nrm), L.ptr(tri), L.ptr(info), L.ptr(ws), nbytes)

    call(0, 0, None, None, None)
    V, T = (int(v) for v in info.cpu().numpy()[:2])
    pos = torch.empty(V, 3, dtype=torch.float32, device=DEV)
    nrm = torch.empty(V, 3, dtype=torch.float32, device=DEV)
    tri = torch.empty(T, 3, dtype=torch.int32, device=DEV)
    full = profiled(lib, lambda: call(V, T, pos, nrm, tri), a.reps, ["surface_extract"])["surface_extract"][0]
    dense = profiled(lib, lambda: call(0, 0, None, None, None), a.reps, ["surface_extract"])["surface_extract"][0]
    assert info.cpu().numpy().tolist() == [V, T, V, T]
    lattice_bytes = 4 * n ** 3
    floor = 1e3 * lattice_bytes / COPY_BW
    mesh = SF.SurfaceMesh(pos, nrm, tri, None)
    got = mesh.measure()
    R = 0.36 * n
    say(f"# surface mesh: each device figure is the mean of {a.reps} calls between mnf_profile_begin and mnf_profile_end (hipEvent pairs per label), after 2 warm-up calls")
    say(f"extract  {n}^3 ball lattice ({lattice_bytes / 1e6:.1f} MB of values, workspace {nbytes / 1e6:.1f} MB): {V} vertices, {T} triangles; "
        f"area / exact {got['area'] / (4 * np.pi * R * R):.5f}, volume / exact {got['volume'] / (4 / 3 * np.pi * R ** 3):.5f}")
    say(f"extract  surface_extract {full:8.3f} ms | the lattice's bytes at 6.29 TB/s: {floor:.3f} ms -> ratio {full / floor:.2f}")
    say(f"extract  the same call with capacities 0 (count pass, two scans, emit pass that writes nothing): {dense:8.3f} ms = {dense / floor:.2f} x the floor; "
        f"the dense passes move 12 B per lattice point (4 B values read, 4 B words written, 4 B words read) = 3.00 x the floor's bytes")
    say(f"extract  vertices and triangles on top: {full - dense:8.3f} ms for {V * 24 + T * 12} B written ({(V * 24 + T * 12) / lattice_bytes:.4f} x the lattice's bytes), "
        f"14 value loads per vertex for its two gradients, 6 word / scan loads per triangle")
    del values, ws, pos, nrm, tri
    if a.extract_only:
        return
    # ---- 2. the lattice fill of the stand-in
    scene = SC.make_scene("102344250", n_poses=8)
    field, est, _ = ST.train_standin(scene, DEV)
    b = est.binaries[0]
    shape = tuple(int(x) * a.refine + 1 for x in b.shape)
    holder = {}

    def fill():
        holder["lattice"] = SF.lattice_from_field(field, est, a.refine)

    res = profiled(lib, fill, a.reps, ["surface_lattice_points", "field_density", "surface_lattice_scatter"])
    vals, origin, step = holder["lattice"]
    listed = int(SF.lattice_points(b, a.refine, est.aabbs[0])["lin"].shape[0])
    pts_n = int(np.prod(shape))
    say(f"fill     stand-in of scene 102344250, grid {tuple(b.shape)} with {int(b.sum())} occupied cells, refine {a.refine}: lattice {shape} = {pts_n} points, "
        f"{listed} listed ({100.0 * listed / pts_n:.1f} %)")
    for label in ("surface_lattice_points", "field_density", "surface_lattice_scatter"):
        say(f"fill     {label:26s} {res[label][0]:8.3f} ms per fill ({res[label][1]:.0f} bracketed launches; lattice_from_field lists twice: once to count)")
    say(f"fill     density queries: {listed / max(res['field_density'][0], 1e-9) / 1e6:.2f} G points/s")
    # ---- 3. the whole route
    iso = 1e-2 / SC.RENDER_KW["render_step_size"]
    ts = []
    for _ in range(a.reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m = SF.extract_surface(field, est, iso, refine=a.refine)
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
    say(f"wall     extract_surface(refine={a.refine}, iso={iso:g}): median {np.median(ts[1:]):8.3f} ms ({min(ts[1:]):.3f}-{max(ts[1:]):.3f}) of {a.reps} calls "
        f"(host clock, synchronised); {m.n_vertices} vertices, {m.n_triangles} triangles, {len(torch.unique(m.label))} classes among the labels")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
