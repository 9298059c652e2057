"""Measurement of one pose-refinement iteration (profiles/pose_refine_step.txt) on the `train_refyaml` scene (102344280, trained stand-in),
at the reference yaml's 2000 rays and at 8192 rays.  One iteration: `transform_rays` of a fixed batch by the 6-vector being optimised, the train render,
L2 photometric loss against the batch's pixels, `loss.backward()`, `torch.optim.Adam` on the six numbers.  The map is not updated in any leg.

  (a)  frozen parameters, `fused_train_render`: the hand-over to the call-by-call drop-in, the only route before `fused_train_render_rays`
  (b)  trainable parameters, `fused_train_render_rays`: the fused backward with every parameter gradient, then the ray kernel
  (c)  frozen parameters, `fused_train_render_rays`: the fused backward without weight gradients and hash scatter, then the ray kernel

One process; the legs are interleaved repetition by repetition; ms per iteration, median with min-max over the repetitions (tools/train_render_measure.py's
manner).  A separate pass per leg between `mnf_profile_begin` / `mnf_profile_end` gives the library's per-label kernel times (hipEvent pairs; they
serialise the side streams, so they are not added up to the iteration time).

    python tools/pose_refine_measure.py [--reps 5] [--steps 20] [--rays 2000,8192] [--out FILE]

The table goes to profiles/pose_refine_step.txt unless `--out` names another file.
"""
import argparse
import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import bench as B  # noqa: E402  (the harness: Ctx, TrainLeg)

LABELS = ("sample_rays", "field_density", "field_train_forward", "composite_train_forward", "composite_train_backward", "dgrad", "wgrad", "hash_scatter",
          "hash_scatter_bins", "field_input_grad", "train_render_ray_grad")
XI0 = (0.01, -0.02, 0.015, 0.02, -0.01, 0.015)


def pose_leg(cx, tl, R_, ray_gradients, frozen):
    from apnrf_amd import render as RD
    from apnrf_amd import scenes as SC
    torch = cx.torch
    tf, te, _ = tl.fresh_member(optimizer="torch")
    for prm in tf.parameters():
        prm.requires_grad_(not frozen)
    rays, pixels, _, _ = tl.make_batches(R_)[0]
    bkd = torch.rand(3, generator=torch.Generator().manual_seed(7)).to(cx.dev)
    xi = torch.tensor(XI0, device=cx.dev, requires_grad=True)
    optimizer = torch.optim.Adam([xi], lr=1e-3)
    stats = {"n": []}

    def step(i):
        optimizer.zero_grad()
        moved = RD.transform_rays(rays, xi[:3], xi[3:])
        render = RD.fused_train_render_rays if ray_gradients else RD.fused_train_render
        rgb, _, _, _, n = render(tf, te, moved, render_bkgd=bkd, **SC.RENDER_KW)
        loss = ((rgb - pixels) ** 2).mean()
        loss.backward()
        optimizer.step()
        if not frozen:
            tf.zero_grad(set_to_none=True)      # (the map is not updated: its gradients are computed and dropped)
        stats["n"].append(n)
        return loss
    return step, stats


def kernel_times(cx, step, iters):
    """us per iteration and launches per iteration of every label, from one profiled pass"""
    lib = cx.lib
    cx.torch.cuda.synchronize()
    lib.mnf_profile_begin()
    for i in range(iters):
        step(i)
    cx.torch.cuda.synchronize()
    lib.mnf_profile_end(None, None)
    out = []
    for label in LABELS:
        ms, cnt = ctypes.c_double(), ctypes.c_int64()
        lib.mnf_profile_query(label.encode(), ctypes.byref(ms), ctypes.byref(cnt))
        if cnt.value:
            out.append(f"{label} {1e3 * ms.value / iters:.0f} us x {cnt.value / iters:g}")
    return ", ".join(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rays", default="2000,8192")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(HERE), "profiles", "pose_refine_step.txt"))
    a = ap.parse_args()
    assert a.reps >= 1 and a.reps * a.steps >= 50, "medians over at least 50 iterations"
    cx = B.Ctx(B.parse(["--gpus", "1", "--workload", "train", "--warmup", "6", "--no-cpu-baseline"]))
    tl = B.TrainLeg(cx, "102344280", seed=11)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# pose-refinement iteration: scene 102344280 (trained stand-in, the map never updated), {a.reps} interleaved repetitions of {a.steps} iterations after "
        f"warm-up; ms per iteration, median (min-max); device {cx.torch.cuda.get_device_name(0)}")
    say("# one iteration: transform_rays(batch, xi) -> fused_train_render -> ((rgb - pixels) ** 2).mean() -> backward -> torch.optim.Adam([xi]); kernel lines: "
        "the library's hipEvent pairs per label in a pass of their own, us per iteration x launches per iteration")
    for R_ in [int(x) for x in a.rays.split(",")]:
        legs = {
            "a": ("(a)  frozen parameters, fused_train_render: the hand-over to the drop-in", lambda: pose_leg(cx, tl, R_, False, True)),
            "b": ("(b)  trainable parameters, fused_train_render_rays", lambda: pose_leg(cx, tl, R_, True, False)),
            "c": ("(c)  frozen parameters, fused_train_render_rays", lambda: pose_leg(cx, tl, R_, True, True)),
        }
        made = {k: (label,) + make() for k, (label, make) in legs.items()}
        times = {k: [] for k in made}
        for rep in range(a.reps):
            for k, (label, step, stats) in made.items():
                times[k].append(1e3 * cx.timed(step, a.steps, 8 if rep == 0 else 2, False) / a.steps)
        say(f"## {R_} rays per iteration")
        for k, (label, step, stats) in made.items():
            t = times[k]
            say(f"{label:80s} {np.median(t):7.3f} ms ({min(t):.3f}-{max(t):.3f})  samples per iteration {np.mean(stats['n'][-a.steps:]):9.0f}")
        for k, (label, step, stats) in made.items():
            say(f"     ({k}) kernels: {kernel_times(cx, step, 10)}")
        ta, tc = times["a"], times["c"]
        say(f"(a) - (c) = {np.median(ta) - np.median(tc):.3f} ms; (a)'s own min-max spread {max(ta) - min(ta):.3f} ms, (c)'s {max(tc) - min(tc):.3f} ms")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
