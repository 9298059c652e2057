"""Measurement of one pose-refinement iteration (profiles/pose_refine_step.txt and profiles/pose_refine_batch.txt) on the `train_refyaml` scene (102344280, trained stand-in),
at the reference yaml's 2000 rays and at 8192 rays.  One iteration: `transform_rays` of a fixed batch by the 6-vector being optimised, the train render,
L2 photometric loss against the batch's pixels, `loss.backward()`, `torch.optim.Adam` on the six numbers.  The map is not updated in any leg.

  (a)  frozen parameters, `fused_train_render`: the hand-over to the call-by-call drop-in, the only route before `fused_train_render_rays`
  (b)  trainable parameters, `fused_train_render_rays`: the fused backward with every parameter gradient, then the ray kernel
  (c)  frozen parameters, `fused_train_render_rays`: the fused backward without weight gradients and hash scatter, then the ray kernel
  (d)  the batched refiner (`localize.PoseRefiner`, `mnf_pose_refine`) on ONE view with as many rays as (c): pixels drawn, rays formed, rendered, the
       three-term loss, the frozen backward and Adam on the device; timed as one C call per iteration and as one C call for the whole run
  (e)  the refiner on 8 views of an eighth of the rays each (at ray counts of 8192 and more): per view against (c)

(d) and (e) read their targets from a `Dataset` of eight 160 x 160 images (the stand-in's analytic targets at the batches' poses) and use the refiner's
three-term loss where (a)-(c) take an L2 photometric loss on a fixed batch; the render behind them is the same call.

One process; the legs are interleaved repetition by repetition; ms per iteration, median with min-max over the repetitions (tools/train_render_measure.py's
manner).  A separate pass per leg between `mnf_profile_begin` / `mnf_profile_end` gives the library's per-label kernel times (hipEvent pairs; they
serialise the side streams, so they are not added up to the iteration time).

    python tools/pose_refine_measure.py [--reps 5] [--steps 20] [--rays 2000,8192] [--legs abcde] [--out FILE]

The table goes to profiles/pose_refine_batch.txt unless `--out` names another file (`--legs abc --out profiles/pose_refine_step.txt` is the earlier table).
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
          "hash_scatter_bins", "field_input_grad", "train_render_ray_grad", "pose_rays", "pose_loss", "pose_update")
SIDE = 160      # the refiner legs' images
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


def refiner_dataset(cx, tl):
    """Eight SIDE x SIDE captures at the batches' poses with the stand-in's analytic targets, as a `Dataset` on the device"""
    from apnrf_amd import render as RD
    from apnrf_amd import standin as SI
    from apnrf_amd.dataset import Dataset
    torch = cx.torch
    K = np.array([[SIDE / 2.0, 0, SIDE / 2.0], [0, SIDE / 2.0, SIDE / 2.0], [0, 0, 1.0]])
    r = RD.generate_image_rays(torch.from_numpy(tl.c2w), SIDE, SIDE, K, cx.dev)
    o, d = r.origins.reshape(-1, 3), r.viewdirs.reshape(-1, 3)
    parts = [SI.analytic_targets(tl.proc, tl.scene["aabb"], o[i:i + 8192], d[i:i + 8192]) for i in range(0, o.shape[0], 8192)]      # (the batch size the stand-in trains with)
    pix, dep, lab = (torch.cat([p[k] for p in parts]) for k in range(3))
    V = tl.c2w.shape[0]
    ds = Dataset(training=False, save_fp="", device=cx.dev)
    ds.update_data((pix.view(V, SIDE, SIDE, 3).clamp(0, 1) * 255).round().to(torch.uint8), dep.view(V, SIDE, SIDE), lab.view(V, SIDE, SIDE), torch.from_numpy(tl.c2w))
    return ds


def refiner_leg(cx, tl, ds, B, n):
    """-> (run(k): enqueue k iterations as ONE call, stats).  The corrections start at XI0 and keep moving, as the torch legs' do; the map is frozen."""
    from apnrf_amd import scenes as SC
    from apnrf_amd.localize import PoseRefiner
    tf, te, _ = tl.fresh_member(optimizer="torch")
    tf.requires_grad_(False)
    ref = PoseRefiner(tf, te, ds, list(range(B)), rays_per_view=n, lr_rot=1e-3, lr_trans=1e-3, seed=7, **SC.RENDER_KW)
    ref.xi.copy_(cx.torch.tensor([XI0] * B, dtype=cx.torch.float64))
    return ref.step, ref


def timed_run(cx, run, steps, warmup):
    """seconds of ONE call that enqueues `steps` iterations, after a call of `warmup`"""
    import gc
    import time
    run(warmup)
    gc.collect()
    cx.torch.cuda.synchronize()
    t0 = time.perf_counter()
    run(steps)
    cx.torch.cuda.synchronize()
    return time.perf_counter() - t0


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
    ap.add_argument("--legs", default="abcde")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(HERE), "profiles", "pose_refine_batch.txt"))
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
    if set(a.legs) & set("de"):
        say(f"# (d), (e): localize.PoseRefiner on {SIDE} x {SIDE} captures, pixels drawn on the device, three-term loss, Adam on the device; 'per call': one mnf_pose_refine call "
            f"per iteration, 'per run': one call for the {a.steps} iterations; no host synchronisation inside either")
        ds = refiner_dataset(cx, tl)
    for R_ in [int(x) for x in a.rays.split(",")]:
        legs = {
            "a": ("(a)  frozen parameters, fused_train_render: the hand-over to the drop-in", lambda: pose_leg(cx, tl, R_, False, True)),
            "b": ("(b)  trainable parameters, fused_train_render_rays", lambda: pose_leg(cx, tl, R_, True, False)),
            "c": ("(c)  frozen parameters, fused_train_render_rays", lambda: pose_leg(cx, tl, R_, True, True)),
        }
        made = {k: (label,) + make() for k, (label, make) in legs.items() if k in a.legs}
        times = {k: [] for k in made}
        shapes = ([(1, R_)] if "d" in a.legs else []) + ([(8, R_ // 8)] if "e" in a.legs and R_ >= 8192 and R_ % 8 == 0 else [])
        refiners = {(nv, n): refiner_leg(cx, tl, ds, nv, n) for nv, n in shapes}
        r_call, r_run = {k: [] for k in refiners}, {k: [] for k in refiners}
        for rep in range(a.reps):
            for k, (label, step, stats) in made.items():
                times[k].append(1e3 * cx.timed(step, a.steps, 8 if rep == 0 else 2, False) / a.steps)
            for k, (run, ref) in refiners.items():
                r_call[k].append(1e3 * cx.timed(lambda i: run(1), a.steps, 8 if rep == 0 else 2, False) / a.steps)
                r_run[k].append(1e3 * timed_run(cx, run, a.steps, 2) / a.steps)
        say(f"## {R_} rays per iteration")
        for k, (label, step, stats) in made.items():
            t = times[k]
            say(f"{label:80s} {np.median(t):7.3f} ms ({min(t):.3f}-{max(t):.3f})  samples per iteration {np.mean(stats['n'][-a.steps:]):9.0f}")
        for k, (label, step, stats) in made.items():
            say(f"     ({k}) kernels: {kernel_times(cx, step, 10)}")
        for (nv, n), (run, ref) in refiners.items():
            name = "(d)" if nv == 1 else "(e)"
            out = ref.result()
            kept = out["counts"][-a.steps:, 1].mean()
            for what, t in (("per call", r_call[(nv, n)]), ("per run", r_run[(nv, n)])):
                label = f"{name}  PoseRefiner, {nv} view{'s' if nv > 1 else ''} x {n} rays, {what}"
                say(f"{label:80s} {np.median(t):7.3f} ms ({min(t):.3f}-{max(t):.3f})  samples per iteration {kept:9.0f}"
                    + (f"  = {np.median(t) / nv:.3f} ms per view" if nv > 1 else ""))
            say(f"     {name} stalled iterations {out['stalled'].tolist()}, status bits {out['status']}")
            say(f"     {name} kernels: {kernel_times(cx, lambda i: run(1), 10)}")
        if "a" in made and "c" in made:
            ta, tc = times["a"], times["c"]
            say(f"(a) - (c) = {np.median(ta) - np.median(tc):.3f} ms; (a)'s own min-max spread {max(ta) - min(ta):.3f} ms, (c)'s {max(tc) - min(tc):.3f} ms")
        if "c" in made:
            tc = times["c"]
            for (nv, n), t in r_run.items():
                say(f"(c) - {'(d)' if nv == 1 else '(e) per view'} per run = {np.median(tc) - np.median(t) / nv:.3f} ms of (c)'s {np.median(tc):.3f} ms; (c)'s own min-max spread "
                    f"{max(tc) - min(tc):.3f} ms, the refiner's {(max(t) - min(t)) / nv:.3f} ms")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
