"""Measurement of the 8-bit frame route (profiles/frames_vs_host.txt): the frames of `--poses` poses at `--size` x `--size`,
C = 29, of the bench stand-in (scene 102344529), made two ways in one process, the legs alternating repetition by repetition:

  host route    `render_image_from_pose` (float64 host stacks) followed by the numpy expressions of pipeline.py:994-1022 per pose
                (np.float32(rgb * 255), np.clip(dep * 25, 0, 255), acc * 255, np.argmax, the palette, the channel flip) and the narrowing
                to uint8 that cv2.imwrite does (np.rint of the clipped value)
  device route  `render_frames`: the same renders, `mnf_frames_views` on the device, one uint8 copy to the host

plus the shared render alone (`render_views`, rays resident), `mnf_frames_views`' own time from the library's hipEvent pairs
(`mnf_profile_begin/end`, label "frames_views") with the bytes per second its algorithmic byte count gives, and the bytes handed to the
host per pose by either route.  Both routes' frames are compared byte for byte before anything is timed.

    python tools/bench_frames.py [--poses 8] [--size 640] [--reps 7] [--out FILE]
"""
import argparse
import ctypes
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import apnrf_amd  # noqa: E402
from apnrf_amd import render as RD  # noqa: E402
from apnrf_amd import scenes as SC  # noqa: E402
from apnrf_amd import standin as ST  # noqa: E402

DEV = "cuda:0"
C = 29


def sat8(x):
    with np.errstate(invalid="ignore"):
        r = np.rint(np.clip(x, 0, 255))
    return np.where(np.isnan(r), 0, r).astype(np.uint8)


def host_route(args, palette):
    """The parent route: float64 stacks to the host, then pipeline.py:976-1023 per pose."""
    images, depths, accs, sems = RD.render_image_from_pose(*args, None, DEV)
    out = dict(rgb=[], depth=[], occ=[], sem=[])
    for i in range(images.shape[0]):
        out["rgb"].append(sat8(np.float32(images[i] * 255))[..., ::-1])
        out["depth"].append(sat8(np.clip(depths[i] * 25, 0, 255)))
        out["occ"].append(sat8(accs[i] * 255))
        out["sem"].append(palette[np.argmax(sems[i], axis=-1)][..., ::-1])
    return {k: np.stack(v) for k, v in out.items()}


def host_route_split(args, palette, reps):
    """Where the host route's time goes: the render with its float64 hand-over, and the numpy conversion alone (argmax apart)."""
    t = dict(render_and_handover=[], argmax=[], rest=[])
    for _ in range(reps):
        t0 = time.perf_counter()
        images, depths, accs, sems = RD.render_image_from_pose(*args, None, DEV)
        t1 = time.perf_counter()
        labels = [np.argmax(sems[i], axis=-1) for i in range(sems.shape[0])]
        t2 = time.perf_counter()
        for i in range(images.shape[0]):
            sat8(np.float32(images[i] * 255))[..., ::-1]; sat8(np.clip(depths[i] * 25, 0, 255)); sat8(accs[i] * 255); palette[labels[i]][..., ::-1]
        t3 = time.perf_counter()
        t["render_and_handover"].append(1e3 * (t1 - t0)); t["argmax"].append(1e3 * (t2 - t1)); t["rest"].append(1e3 * (t3 - t2))
    return {k: float(np.median(v)) for k, v in t.items()}


def timed(fn):
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--poses", type=int, default=8)
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    if not torch.cuda.is_available():
        raise SystemExit("bench_frames.py measures on the GPU: no device found")
    lib = apnrf_amd.load_library()
    N, S = a.poses, a.size
    scene = SC.make_scene("102344529", n_poses=max(8, N))
    field, est, _ = ST.train_standin(scene, DEV)
    poses = scene["poses"][:N]
    focal = 0.5 * S / np.tan(np.pi / 4)
    kw = SC.RENDER_KW
    args = (field, est, poses, S, S, focal, kw["near_plane"], kw["render_step_size"], 1, kw["cone_angle"], kw["alpha_thre"])
    palette = np.random.default_rng(0).integers(0, 256, (40, 3), dtype=np.uint8)
    P = S * S
    say(f"# 8-bit frames of {N} poses at {S}x{S}, C = {C}, trained stand-in of scene 102344529, {torch.cuda.get_device_name(0)}; "
        f"{a.reps} alternating repetitions per leg after one warm-up of each")

    want, got = host_route(args, palette), RD.render_frames(*args, palette, device=DEV)         # warm-up of both legs, and the check
    same = {k: bool(np.array_equal(want[k], got[k])) for k in want}
    say(f"frames of the two routes equal byte for byte: {same}")
    if not all(same.values()):
        raise SystemExit("the routes disagree: nothing is timed")
    o, d, h, w = RD._pose_rays(poses, S, S, focal, 1, DEV)

    def render_only():
        RD.render_views(field, est, o, d, P, 1024, near_plane=kw["near_plane"], render_step_size=kw["render_step_size"], render_bkgd=torch.zeros(3),
                        cone_angle=kw["cone_angle"], alpha_thre=kw["alpha_thre"], image_hw=(h, w), n_split=None)

    legs = {"host route (render_image_from_pose + numpy)": lambda: host_route(args, palette),
            "device route (render_frames)": lambda: RD.render_frames(*args, palette, device=DEV),
            "device route, views_per_call=8": lambda: RD.render_frames(*args, palette, views_per_call=8, device=DEV),
            "the renders alone (one call, rays resident)": render_only}
    render_only()
    legs["device route, views_per_call=8"]()
    times = {k: [] for k in legs}
    for _ in range(a.reps):
        for k, fn in legs.items():
            times[k].append(timed(fn))
    for k, ts in times.items():
        ts = np.asarray(ts) / N
        say(f"wall per pose  {k:46s} median {np.median(ts):8.2f} ms  min {ts.min():8.2f}  max {ts.max():8.2f}")
    host_med, dev_med = (np.median(times[k]) for k in list(legs)[:2])
    say(f"host route / device route = {host_med / dev_med:.2f}x")
    split = host_route_split(args, palette, max(3, a.reps // 2))
    say("host route per pose, medians: " + ", ".join(f"{k} {v / N:.2f} ms" for k, v in split.items()))

    r = RD.render_views(field, est, o, d, P, 1024, near_plane=kw["near_plane"], render_step_size=kw["render_step_size"], render_bkgd=torch.zeros(3),
                        cone_angle=kw["cone_angle"], alpha_thre=kw["alpha_thre"], image_hw=(h, w), n_split=None)
    planes = (r["rgb"].view(N, P, 3), r["depth"].view(N, P), r["acc"].view(N, P), r["sem"].view(N, P, C))
    for labels in (False, True):
        for _ in range(3):
            RD.frames_from_renders(*planes, palette, labels=labels)
        torch.cuda.synchronize()
        lib.mnf_profile_begin()
        for _ in range(20):
            RD.frames_from_renders(*planes, palette, labels=labels)
        lib.mnf_profile_end(None, None)
        ms, n = ctypes.c_double(), ctypes.c_int64()
        lib.mnf_profile_query(b"frames_views", ctypes.byref(ms), ctypes.byref(n))
        per_call = ms.value / max(n.value, 1)
        nbytes = ((3 + 1 + 1 + C) * 4 + 8 + int(labels)) * N * P            # the algorithmic byte count of DESIGN.md §4.6
        tbs = nbytes / (per_call * 1e-3) / 1e12
        say(f"mnf_frames_views labels={int(labels)}: {1e3 * per_call:8.1f} us per call of {N} views ({n.value} calls, hipEvents), "
            f"{nbytes // (N * P)} B per pixel -> {tbs:.2f} TB/s = {tbs / 8.0:.3f} of 8 TB/s")
    say(f"bytes handed to the host per pose: host route {P * (3 + 1 + 1 + C) * 8} (float64 stacks), device route {P * 8} (uint8 planes)")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
