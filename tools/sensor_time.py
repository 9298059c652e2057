"""Measurement of the scene sensor (DESIGN.md "Scene sensor", profiles/sensor.txt).

  build    the ground-truth world of scene 102344250 at refine 4 (the procedural rooms at 5 cm): the host builder (`sensor.occupancy_words`,
           once, a host clock), the copy to the device and `mnf_sensor_build_bricks` (device events).
  views    `VoxelSim.render_c2w` for the 40 poses of the reference's first yaw sweep at 640 x 640, planar and ray depth, with and without the
           hit plane: device events, medians (min-max) after warm-ups, and the rays per second that makes; the brick mask's size and fill.
  standin  `standin.analytic_targets`, what stood in for a sensor until now, on rays of the same 40 views: the library's marcher at 1 mm steps
           over the 0.2 m procedural grid.  It builds every sample of a ray before it picks the first, so it is run as the stand-in's
           training runs it, 8192 rays a call, on 64 such batches drawn evenly from the 16.4 M rays; the figure is per ray.

The walk is the plain one: it steps every voxel and loads `voxels` only inside bricks whose bit is set.  There is no brick-stride variant
to measure.  Every GPU step is a child process of its own under `timeout`; the driver starts no GPU work itself, stops at the first step
that fails and writes what the steps printed.  There is no pass/fail gate on a time.

    python tools/sensor_time.py [--reps 9] [--out profiles/sensor.txt]
"""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

DEV = "cuda:0"
SCENE, REFINE, VIEWS, SIDE = "102344250", 4, 40, 640
STEPS = (("build", 240), ("views", 300), ("standin", 300))


def fmt(t):
    return f"{t[0]:9.3f} ms ({t[1]:.3f}-{t[2]:.3f})"


def world():
    from apnrf_amd import scenes as SC
    from apnrf_amd import sensor as SN
    scene = SC.make_scene(SCENE, n_poses=VIEWS)
    t0 = time.perf_counter()
    words, lo, s = SN.occupancy_words(scene["occ"], scene["aabb"], refine=REFINE, closed=True)
    return scene, words, lo, s, time.perf_counter() - t0


def step_build(reps):
    import torch
    from apnrf_amd import sensor as SN
    from object_map_measure import event_ms
    scene, words, lo, s, host_s = world()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    vs = SN.VoxelScene(words, lo, s, device=DEV)
    torch.cuda.synchronize()
    up_s = time.perf_counter() - t0
    ms = event_ms({"bricks": (None, vs.rebuild)}, reps, warmup=3)
    bits = int(sum(bin(int(w) & 0xFFFFFFFF).count("1") for w in vs.bricks.cpu().numpy()))
    n_bricks = int(np.prod([(n + 7) // 8 for n in vs.shape]))
    print(f"build      scene {SCENE} at refine {REFINE}: {vs.shape[0]} x {vs.shape[1]} x {vs.shape[2]} voxels of {s * 100:.0f} cm ({words.nbytes / 2 ** 20:.0f} MiB), "
          f"{int(((words >> 24) != 0xFF).sum())} occupied; brick mask {vs.bricks.numel()} words ({vs.bricks.numel() * 4} B of LDS), {bits} of {n_bricks} bricks set"
          f" | host builder {host_s:.2f} s (once); copy up + first mask {up_s * 1e3:.1f} ms (once); mnf_sensor_build_bricks {fmt(ms['bricks'])}"
          f" = {words.nbytes / ms['bricks'][0] * 1e-6:.0f} GB/s of voxel words")


def step_views(reps):
    import torch
    from apnrf_amd import render as RD
    from apnrf_amd import sensor as SN
    from object_map_measure import event_ms
    scene, words, lo, s, _ = world()
    vs = SN.VoxelScene(words, lo, s, device=DEV)
    sim = SN.VoxelSim(vs, SIDE, SIDE)
    c2w = torch.from_numpy(np.stack([RD.pose_to_c2w(p) for p in scene["poses"]])[:, :3, :]).to(DEV)
    legs = {"planar": (None, lambda: sim.render_c2w(c2w)), "ray": (None, lambda: sim.render_c2w(c2w, depth="ray")),
            "planar+hit": (None, lambda: sim.render_c2w(c2w, hit=True))}
    ms = event_ms(legs, reps, warmup=2)
    sim.clear_info()
    out = sim.render_c2w(c2w)
    misses = int(sim.info[0])
    rays = VIEWS * SIDE * SIDE
    depth = out["depth"]
    out_bytes = rays * (4 + 4 + 1)
    print(f"views      {VIEWS} views of {SIDE} x {SIDE} ({rays / 1e6:.1f} M rays, {misses} misses, mean depth {float(depth.mean()):.2f} m = "
          f"{float(depth.mean()) / s:.0f} voxels): planar {fmt(ms['planar'])} = {rays / ms['planar'][0] * 1e-6:.2f} G rays/s; ray depth {fmt(ms['ray'])}; "
          f"with the hit plane {fmt(ms['planar+hit'])}; the images are {out_bytes / 2 ** 20:.0f} MiB: {out_bytes / ms['planar'][0] * 1e-6:.1f} GB/s of stores")


def step_standin(reps):
    import torch
    from apnrf_amd import render as RD
    from apnrf_amd import scenes as SC
    from apnrf_amd import standin as ST
    from object_map_measure import event_ms
    scene = SC.make_scene(SCENE, n_poses=VIEWS)
    proc = ST._procedural_estimator(scene, DEV)
    c2w = np.stack([RD.pose_to_c2w(p) for p in scene["poses"]]).astype(np.float32)
    focal = 0.5 * SIDE / np.tan(np.pi / 4)
    K = np.array([[focal, 0, SIDE / 2], [0, focal, SIDE / 2], [0, 0, 1.0]])
    batch, n_batches = 8192, 64
    rng = np.random.default_rng(0)
    rays = []
    for b in range(n_batches):
        idx = np.sort(rng.choice(SIDE * SIDE, batch, replace=False))
        rays.append(RD.generate_image_rays(torch.from_numpy(c2w[b % VIEWS:b % VIEWS + 1]), SIDE, SIDE, K, DEV, idx))

    def run():
        for r in rays:
            ST.analytic_targets(proc, scene["aabb"], r.origins, r.viewdirs)
    ms = event_ms({"standin": (None, run)}, max(3, reps // 3), warmup=1)
    n = batch * n_batches
    per_ray_ns = ms["standin"][0] * 1e6 / n
    print(f"standin    standin.analytic_targets on {n_batches} batches of {batch} rays of the same views ({n / 1e6:.2f} M rays): {fmt(ms['standin'])} = "
          f"{per_ray_ns:.1f} ns per ray, {per_ray_ns * VIEWS * SIDE * SIDE * 1e-6:.0f} ms for the {VIEWS * SIDE * SIDE / 1e6:.1f} M rays of the {VIEWS} views at that rate "
          f"(0.2 m cells and a + 0.02 m fudge, not 5 cm voxels: not the same answer)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", default=None, help="(internal) run one GPU step in this process")
    a = ap.parse_args()
    if a.step:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("sensor_time needs a GPU: nothing here is a measurement without one")
        import apnrf_amd  # noqa: F401
        {"build": step_build, "views": step_views, "standin": step_standin}[a.step](a.reps)
        return
    lines = [f"# scene sensor; medians of {a.reps} repetitions (min-max) after warm-ups, device events around each call; host figures are this machine's CPU "
             f"({os.cpu_count()} CPUs, numpy {np.__version__}).  The plain walk (every voxel stepped, voxels loaded in set bricks only); no speed bar was set beforehand."]
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
