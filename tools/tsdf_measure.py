"""Measurement of TSDF fusion (DESIGN.md "TSDF fusion", profiles/tsdf_fusion.txt): 40 views of 640 x 640 of the ground-truth world of scene
102344250 (the procedural rooms at 5 cm, `VoxelSim`, planar depth, RGBA and uint8 classes as the sensor leaves them) fused into a
`TsdfVolume` at 5 cm over the scene's aabb.

  a  one `mnf_tsdf_integrate` call of 40 views
  b  the same kernel called 40 times with one view each

The two legs are interleaved in one process: every repetition runs a, then b, each between a hipEvent pair, after warm-up repetitions;
the figures are the median and min-max of the repetitions.  Both legs fuse into a volume that already holds the 40 views (the state's
values do not change what is loaded or stored).  Each leg is set against its algorithmic bytes at the device-to-device copy bandwidth of
the microarchitecture guide: 32 B (16 read, 16 written) per touched point per call, a touched point being a point of an aligned 4 x 4 x 16
block in which that call observes at least one point, plus every pixel of the call's views once (4 B depth, 4 B colour, 1 B class).

The block shape is a compile-time constant of csrc/tsdf.hip (MNF_TSDF_BLOCK: 0 = 4 x 4 x 16, 1 = 1 x 4 x 64, 2 = 2 x 8 x 16).  One run
measures the library it loads; a run per experiment build (tools/build_variants.sh "zlong -DMNF_TSDF_BLOCK=1", then
MNF_LIB_PATH=build/variants/lib_zlong.so) with `--label` and `--append` puts every shape that was tried into one file.  The whole
measurement is one child process under `timeout`.  No speed bar was set beforehand and no test holds a speed.

    python tools/tsdf_measure.py [--reps 10] [--label "4 x 4 x 16"] [--out profiles/tsdf_fusion.txt] [--append]
"""
import argparse
import os
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

DEV = "cuda:0"
SCENE, REFINE, VIEWS, SIDE = "102344250", 4, 40, 640
COPY_BW = 6.29e12          # bytes/s: the device-to-device copy the microarchitecture guide measured


def touched_points(weight):
    """Points of the aligned 4 x 4 x 16 blocks that hold an observed point (the lattice padded up to whole blocks does not count twice:
    only points that exist are counted)."""
    import torch
    import torch.nn.functional as F
    obs = (weight > 0).to(torch.float32)[None, None]
    pad = [(-obs.shape[-1]) % 16, (-obs.shape[-2]) % 4, (-obs.shape[-3]) % 4]
    any_ = F.max_pool3d(F.pad(obs, (0, pad[0], 0, pad[1], 0, pad[2])), kernel_size=(4, 4, 16))
    ones = F.avg_pool3d(F.pad(torch.ones_like(obs), (0, pad[0], 0, pad[1], 0, pad[2])), kernel_size=(4, 4, 16)) * (4 * 4 * 16)
    return int((any_ * ones).sum().item())


def fmt(v):
    return f"{np.median(v):9.3f} ms ({min(v):.3f}-{max(v):.3f})"


def child(reps, label):
    import torch
    import apnrf_amd  # noqa: F401
    from apnrf_amd import render as RD
    from apnrf_amd import scenes as SC
    from apnrf_amd import sensor as SN
    from apnrf_amd.tsdf import TsdfVolume
    if not torch.cuda.is_available():
        raise SystemExit("tsdf_measure needs a GPU: nothing here is a measurement without one")
    scene = SC.make_scene(SCENE, n_poses=VIEWS)
    words, lo, s = SN.occupancy_words(scene["occ"], scene["aabb"], refine=REFINE, closed=True)
    world = SN.VoxelScene(words, lo, s, device=DEV)
    sim = SN.VoxelSim(world, SIDE, SIDE)
    c2w = torch.from_numpy(np.stack([RD.pose_to_c2w(p) for p in scene["poses"]])[:, :3, :]).to(DEV)
    out = sim.render_c2w(c2w)
    rgba, depth, sem = out["rgba"], out["depth"], out["sem"]
    vol = TsdfVolume(world.aabb, s, device=DEV)
    n_points = int(np.prod(vol.shape))
    one = lambda v: vol.integrate(depth[v:v + 1], rgba[v:v + 1], sem[v:v + 1], c2w[v:v + 1], sim.focal)

    def leg_a():
        vol.integrate(depth, rgba, sem, c2w, sim.focal)

    def leg_b():
        for v in range(VIEWS):
            one(v)

    # the algorithmic bytes, on fresh volumes: what one call of 40 views touches, and what 40 calls of one view touch
    touched_b = 0
    for v in range(VIEWS):
        vol.clear()
        one(v)
        touched_b += touched_points(vol.weight)
    vol.clear()
    leg_a()
    touched_a = touched_points(vol.weight)
    info, counts = vol.info(), vol.counts()
    pixel_bytes = VIEWS * SIDE * SIDE * 9
    times = {"a": [], "b": []}
    warmup = 2
    for r in range(warmup + reps):
        for name, fn in (("a", leg_a), ("b", leg_b)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if r >= warmup:
                times[name].append(e0.elapsed_time(e1))
    ms = {k: float(np.median(v)) for k, v in times.items()}
    bytes_a, bytes_b = 32 * touched_a + pixel_bytes, 32 * touched_b + pixel_bytes
    spread = {k: max(v) - min(v) for k, v in times.items()}
    gap = ms["b"] - ms["a"]
    verdict = ("the batched call is ahead: the gap exceeds the spread of either leg" if gap > max(spread.values()) else
               "the one-view calls are ahead: the gap exceeds the spread of either leg" if -gap > max(spread.values()) else
               "neither leg is ahead: the gap is within the spread")
    print(f"shape {label}: volume {vol.shape[0]} x {vol.shape[1]} x {vol.shape[2]} points at {s * 100:.0f} cm ({n_points * 16 / 2 ** 20:.0f} MiB of state), "
          f"{VIEWS} views of {SIDE} x {SIDE}; one fusion applies {info['applied']} observations, {100.0 * counts['observed_fraction']:.1f} % of the points observed, "
          f"skips {info['invalid_depth']} invalid depths and {info['behind_surface']} behind the surface")
    print(f"shape {label}: a  one call of {VIEWS} views        {fmt(times['a'])} | touches {touched_a} points: {bytes_a / 1e6:.0f} MB algorithmic = "
          f"{1e3 * bytes_a / COPY_BW:.3f} ms at 6.29 TB/s -> ratio {ms['a'] / (1e3 * bytes_a / COPY_BW):.1f}")
    print(f"shape {label}: b  {VIEWS} calls of one view each    {fmt(times['b'])} | touch {touched_b} points in all: {bytes_b / 1e6:.0f} MB algorithmic = "
          f"{1e3 * bytes_b / COPY_BW:.3f} ms at 6.29 TB/s -> ratio {ms['b'] / (1e3 * bytes_b / COPY_BW):.1f}")
    print(f"shape {label}: b - a = {gap:.3f} ms (spreads {spread['a']:.3f} / {spread['b']:.3f} ms): {verdict}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--label", default="4 x 4 x 16", help="the block shape of the library that is loaded")
    ap.add_argument("--out", default=None)
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--child", action="store_true", help="(internal) measure in this process")
    a = ap.parse_args()
    if a.child:
        child(a.reps, a.label)
        return
    r = subprocess.run(["timeout", "-k", "10", "400", sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps), "--label", a.label],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    body = [ln for ln in r.stdout.splitlines() if ln.startswith("shape ")] if r.returncode == 0 else r.stdout.splitlines()[-15:] + [f"# ended with status {r.returncode}"]
    head = [] if a.append else [f"# TSDF fusion: medians of {a.reps} repetitions (min-max) after 2 warm-up repetitions, a hipEvent pair around each leg, the legs interleaved "
                                f"in one process; one block of lines per block shape (one experiment build each).  No speed bar was set beforehand."]
    text = "\n".join(head + body)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a" if a.append else "w") as f:
            f.write(text + "\n")
    if r.returncode != 0:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
