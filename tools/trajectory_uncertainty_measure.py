"""Measurement of the ensemble-disagreement trajectory scorer (profiles/trajectory_uncertainty.txt): the 40 views of a
60-pose trajectory, 64 x 64 pixels sub-sampled from 640 x 640, two members (the trained stand-ins of scene 102344250, seeds 9 and 10:
the scoring legs of bench.py), C = 29.

Legs, interleaved repetition by repetition in one process after warm-up:

  host      the caller's way before this route existed: `render_image_from_pose` per member (float64 host stacks), then the
            numpy / torch-CPU reduction of pipeline.py:861-896
  python    `render.trajectory_uncertainty(one_call=False)`: `_render_jobs` + `ensemble_view_terms`, one [V,4] host copy
  one_call  `render.trajectory_uncertainty(one_call=True)`: `mnf_score_trajectory`, one [V,4] host copy

and `mnf_score_ensemble_views` alone on finished renders, by the library's hipEvent pairs (`mnf_profile_begin/end`, label
"score_ensemble_views": both kernels), with its bytes per pixel (3 M + M + 1 + S C) * 4.

    python tools/trajectory_uncertainty_measure.py [--reps 15] [--out FILE]
"""
import argparse
import ctypes
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import apnrf_amd  # noqa: E402
from apnrf_amd import render as RD  # noqa: E402
from apnrf_amd import scenes as SC  # noqa: E402
from apnrf_amd import standin as ST  # noqa: E402

DEV = "cuda:0"
W = H = 640
SCALE = 0.1


def host_route(fields, ests, trajectory, step, focal):
    """`trajector_uncertainty` as a user of the import swap runs it: per-member host stacks, the reduction on the CPU."""
    kw = SC.RENDER_KW
    poses = trajectory[RD.trajectory_view_indices(len(trajectory))]
    rgbs, deps, accs, sems = [], [], [], []
    for f, e in zip(fields, ests):
        rgb, depth, acc, sem = RD.render_image_from_pose(f, e, poses, W, H, focal, kw["near_plane"], kw["render_step_size"], SCALE, kw["cone_angle"],
                                                         kw["alpha_thre"], 4, DEV)
        rgbs.append(rgb); deps.append(depth); accs.append(acc)
        if not sems:
            sems.append(sem)
    rgbs, deps, sems = np.array(rgbs), np.array(deps), np.array(sems)
    p = F.softmax(torch.from_numpy(sems), dim=-1).numpy()
    entropy = -np.sum(p * np.log(p + 1e-10), axis=-1)
    rows = np.stack([np.clip(np.mean(np.mean(np.var(rgbs, axis=0), axis=-1), axis=(1, 2)) * 4000, 0, 100),
                     np.clip(np.mean(np.var(deps, axis=0), axis=(1, 2)) * 50, 0, 100),
                     np.mean(np.clip(1 / (np.array(accs[0]) + 1e-4) - 1, 0, 10000), axis=(1, 2)),
                     np.clip(np.mean(entropy, axis=(0, 2, 3)) * 50, 0, 100)])
    unc, max_idx = RD.trajectory_uncertainty_from_terms(rows.T, step)
    return unc, max_idx, rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    lib = apnrf_amd.load_library()
    scene = SC.make_scene("102344250", n_poses=8)
    members = [ST.train_standin(scene, DEV, seed=s) for s in (9, 10)]
    fields, ests = [m[0].eval() for m in members], [m[1].eval() for m in members]
    trajectory = np.asarray(ST._free_space_poses(scene, 60, seed=9))
    focal = 0.5 * W / np.tan(np.pi / 4)
    kw = SC.RENDER_KW
    args = (fields, ests, trajectory, 1, W, H, focal, kw["near_plane"], kw["render_step_size"], kw["cone_angle"], kw["alpha_thre"])
    legs = {"host": lambda: host_route(fields, ests, trajectory, 1, focal),
            "python": lambda: RD.trajectory_uncertainty(*args, scale=SCALE, device=DEV, one_call=False),
            "one_call": lambda: RD.trajectory_uncertainty(*args, scale=SCALE, device=DEV, one_call=True)}
    results = {}
    for name, fn in legs.items():
        for _ in range(2):
            results[name] = fn()
    torch.cuda.synchronize()
    times = {name: [] for name in legs}
    for _ in range(a.reps):
        for name, fn in legs.items():
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[name].append(1e3 * (time.perf_counter() - t0))
    V, M, S, C, P = 40, 2, 1, fields[0].num_semantic_classes, int(H * SCALE) * int(W * SCALE)
    say(f"# trajectory uncertainty: {V} views of {int(H * SCALE)}x{int(W * SCALE)} (sub-sampled from {H}x{W}), {M} members, C = {C}, trained stand-ins of "
        f"scene 102344250; medians of {a.reps} interleaved repetitions (min-max)")
    for name in legs:
        t = times[name]
        say(f"wall  {name:9s} {np.median(t):7.2f} ms ({np.min(t):.2f}-{np.max(t):.2f})")
    say(f"ratio host / one_call {np.median(times['host']) / np.median(times['one_call']):.2f}x, python / one_call "
        f"{np.median(times['python']) / np.median(times['one_call']):.2f}x")
    say(f"values  host {results['host'][0]:.9f} | python {results['python'][0]:.9f} | one_call {results['one_call'][0]:.9f}; rows one_call == python bitwise: "
        f"{bool(np.array_equal(results['one_call'][2], results['python'][2]))}; max |rows one_call - host| per row "
        f"{np.abs(results['one_call'][2] - results['host'][2]).max(1)}")
    # the kernel alone on finished renders
    poses = trajectory[RD.trajectory_view_indices(len(trajectory))]
    o, d, h, w = RD._pose_rays(poses, W, H, focal, SCALE, DEV)
    outs = [RD.render_views(f, e, o, d, h * w, 1024, render_bkgd=torch.zeros(3), n_split=None, **kw) for f, e in zip(fields, ests)]
    rgb, dep = torch.stack([r["rgb"].view(V, P, 3) for r in outs]), torch.stack([r["depth"].view(V, P) for r in outs])
    acc, sem = torch.stack([r["acc"].view(V, P) for r in outs]), outs[0]["sem"].view(1, V, P, C).contiguous()
    for _ in range(3):
        RD.ensemble_view_terms(rgb, dep, acc, sem)
    torch.cuda.synchronize()
    lib.mnf_profile_begin()
    for _ in range(50):
        RD.ensemble_view_terms(rgb, dep, acc, sem)
    lib.mnf_profile_end(None, None)
    ms, n = ctypes.c_double(), ctypes.c_int64()
    lib.mnf_profile_query(b"score_ensemble_views", ctypes.byref(ms), ctypes.byref(n))
    per_call = ms.value / max(n.value, 1)
    per_pixel = (3 * M + M + 1 + S * C) * 4
    tbs = per_pixel * V * P / (per_call * 1e-3) / 1e12
    say(f"mnf_score_ensemble_views alone: {1e3 * per_call:8.1f} us per call ({n.value} calls, hipEvents, both kernels), {per_pixel} B read per pixel "
        f"-> {tbs:.3f} TB/s = {tbs / 8.0:.4f} of 8 TB/s")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
