"""Measurement of the per-pixel predictive-information maps (profiles/information_maps.txt): `mnf_score_view_maps`
(csrc/infomap.hip) beside `mnf_score_views` (csrc/render.hip: score_kernel) on the same device stacks, M = 2 members, C = 29 classes,
at two shapes: 256 views of 4096 pixels (a scoring batch of 64 x 64 views) and 4 views of 409 600 pixels (full 640 x 640 views).

Legs, interleaved repetition by repetition in one process after warm-up, each timed by a hipEvent pair around the one call:

  terms      `mnf_score_view_maps` with terms only (the work of `mnf_score_views`, on the new work split)
  maps+heat  `mnf_score_view_maps` with terms, the float64 maps and the heat bytes
  score      `mnf_score_views`, the baseline leg

Reported: median and min-max of the repetitions.  A leg is called ahead of the baseline only when the gap between the medians exceeds the
baseline leg's own spread.  The stacks are seeded random renders (variances in [0, 1), opacities in [0, 1], logits of scale 3): the
kernels' time does not depend on the values.

    python tools/infomap_measure.py [--reps 15] [--out profiles/information_maps.txt]
"""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import apnrf_amd  # noqa: E402
from apnrf_amd import _lib as L  # noqa: E402

DEV = "cuda:0"
M, C = 2, 29
SHAPES = [(256, 4096), (4, 409600)]
HEAT_LO, HEAT_HI = (0.0, 0.0, 0.0, 0.0), (0.5, 0.5, 0.5, 0.5)


def stacks(V, P, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    r = lambda *s: torch.rand(*s, device=DEV, generator=g)
    return r(M, V, P, 3) ** 4, r(M, V, P) ** 4, r(M, V, P), torch.randn(M, V, P, C, device=DEV, generator=g) * 3.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "information_maps.txt"))
    a = ap.parse_args()
    if a.reps < 10:
        ap.error("--reps must be at least 10")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    lib = apnrf_amd.load_library()
    lo, hi = (ctypes.c_double * 4)(*HEAT_LO), (ctypes.c_double * 4)(*HEAT_HI)
    say(f"# information maps: mnf_score_view_maps beside mnf_score_views, M = {M}, C = {C}, {torch.cuda.get_device_name(0)}; hipEvent pairs, "
        f"medians of {a.reps} interleaved repetitions after 3 warm-up rounds (min-max)")
    for V, P in SHAPES:
        rv, dv, ac, sm = stacks(V, P, seed=V)
        terms = torch.empty(V, 4, dtype=torch.float64, device=DEV)
        terms_old = torch.empty_like(terms)
        maps = torch.empty(V, P, 4, dtype=torch.float64, device=DEV)
        heat = torch.empty(V, P, 4, dtype=torch.uint8, device=DEV)
        nbytes = max(int(lib.mnf_score_view_maps_workspace_bytes(V, P, C)), 8)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
        ins = [L.ptr(t) for t in (rv, dv, ac, sm)]
        legs = {
            "terms": lambda: L.launch(lib.mnf_score_view_maps, *ins, M, V, P, C, L.ptr(terms), None, None, None, None, L.ptr(ws), nbytes),
            "maps+heat": lambda: L.launch(lib.mnf_score_view_maps, *ins, M, V, P, C, L.ptr(terms), L.ptr(maps), L.ptr(heat), lo, hi, L.ptr(ws), nbytes),
            "score": lambda: L.launch(lib.mnf_score_views, *ins, M, V, P, C, L.ptr(terms_old)),
        }
        for _ in range(3):
            for fn in legs.values():
                fn()
        torch.cuda.synchronize()
        times = {name: [] for name in legs}
        for _ in range(a.reps):
            for name, fn in legs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                times[name].append(e0.elapsed_time(e1))
        read_b, write_b = (3 + 1 + 1 + C) * M * 4, 32 + 4
        say(f"## {V} views x {P} pixels; {read_b} B read per pixel, {write_b} B written with maps and heat; max |terms - mnf_score_views| = "
            f"{(terms - terms_old).abs().max().item():.3e}")
        med = {name: float(np.median(t)) for name, t in times.items()}
        for name, t in times.items():
            gbs = (read_b + (write_b if name == "maps+heat" else 0)) * V * P / (med[name] * 1e-3) / 1e9
            say(f"{name:10s} {med[name]:8.3f} ms ({np.min(t):.3f}-{np.max(t):.3f})  {V * P / med[name] / 1e3:8.1f} Mpixel/s  {gbs:7.1f} GB/s")
        spread = float(np.max(times["score"]) - np.min(times["score"]))
        for name in ("terms", "maps+heat"):
            gap = med["score"] - med[name]
            verdict = "ahead of" if gap > spread else ("behind" if -gap > spread else "level with")
            say(f"{name} is {verdict} mnf_score_views: gap of the medians {gap:+.3f} ms, spread of the baseline leg {spread:.3f} ms")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
