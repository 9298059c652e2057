"""Measurement of the differentiable fused train render (profiles/train_render_split.txt): what a caller who keeps the reference's own loss
lines pays per iteration on the `train_refyaml` scene (102344280, trained stand-in, every leg continued from the same state), at 2000 and at 8192 rays.

  (a)  the loop of tools/bench_extra.py:_dropin_leg, copied unchanged: `render_image_with_occgrid_with_depth_guide`, torch losses, `loss.backward()`, the
       per-parameter isnan loop, torch.optim.Adam + the reference's scheduler — the baseline
  (b)  the same loop with `fused_train_render` swapped in and nothing else changed; (b+) the same with `optim.FusedAdam` bound to the field; (b++) the loop
       handed to `train_step(loss_fn=...)` (the guard taken on the device: one host round trip less)
  (c)  `train_step(fused=True)` host-synchronous: the floor (the loss inside the one C call)

One process; the legs are interleaved repetition by repetition; medians with min-max over the repetitions.

    python tools/train_render_measure.py [--reps 5] [--steps 40] [--rays 2000,8192] [--only b] [--out FILE]

The table goes to profiles/train_render_split.txt unless `--out` names another file.  `--only LEG`: that leg alone (for a kernel trace of it); it writes no
file unless `--out` is given.
"""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import bench as B  # noqa: E402  (the harness: Ctx, TrainLeg)


def _scheduler(torch, optimizer):
    return torch.optim.lr_scheduler.ChainedScheduler([torch.optim.lr_scheduler.CyclicLR(
        optimizer, base_lr=1e-4, max_lr=2e-4, step_size_up=250, mode="exp_range", gamma=1.0, cycle_momentum=False)])   # pipeline.py:183-193's form


def reference_loop(cx, tl, R_, render, fused_adam=False):
    """tools/bench_extra.py:_dropin_leg's step with `render` as the train render (the drop-in, or `fused_train_render` under its name)."""
    import torch.nn.functional as F
    from apnrf_amd import nerfacc as NA
    from apnrf_amd.optim import FusedAdam
    torch = cx.torch
    tf, te, _ = tl.fresh_member(optimizer="torch")
    if fused_adam:
        optimizer = FusedAdam(tf.parameters(), lr=2e-4, eps=1e-15).bind_field(tf)
    else:
        optimizer = torch.optim.Adam(tf.parameters(), lr=2e-4, eps=1e-15, weight_decay=0.0)                      # pipeline.py:173-178
    scheduler = _scheduler(torch, optimizer)
    occ_eval_fn = NA.FieldDensityOcc(tf, 1e-3)                                                                   # pipeline.py:376-378
    batches = tl.make_batches(R_)
    bkd = torch.rand(3, generator=torch.Generator().manual_seed(7)).to(cx.dev)
    stats = {"n": [], "jumped": 0}

    def step(i):
        rays_, pixels, dep_, sem_ = batches[i % 8]
        te.update_every_n_steps(step=1000 + i, occ_eval_fn=occ_eval_fn, occ_thre=1e-2)
        rgb, acc, depth, semantic, n_rendering_samples = render(
            tf, te, rays_, near_plane=0.1, render_step_size=1e-3, render_bkgd=bkd, cone_angle=0.004, alpha_thre=0.01, depth=dep_)
        if n_rendering_samples == 0:
            return None
        loss_rgb = F.smooth_l1_loss(rgb, pixels)
        loss_dep = F.smooth_l1_loss(depth, dep_.unsqueeze(1))
        loss_sem = F.cross_entropy(semantic, sem_)
        loss = loss_rgb * 10 + loss_dep / 5 + loss_sem / 2
        host_losses = (loss_rgb.detach().cpu().item(), loss_dep.detach().cpu().item() / 50, loss_sem.detach().cpu().item() / 2)   # pipeline.py:513-515
        optimizer.zero_grad()
        loss.backward()
        flag = False
        for name, param in tf.named_parameters():
            if param.grad is not None and torch.sum(torch.isnan(param.grad)) > 0:
                flag = True
                break
        if flag:
            optimizer.zero_grad()
            stats["jumped"] += 1
            return None
        optimizer.step()
        scheduler.step()
        stats["n"].append(n_rendering_samples)
        return host_losses
    return step, stats


def train_step_leg(cx, tl, R_, loss_fn=None):
    import torch.nn.functional as F
    from apnrf_amd import render as RD
    from apnrf_amd import scenes as SC
    torch = cx.torch
    tf, te, opt = tl.fresh_member()
    batches = tl.make_batches(R_)
    bkd = torch.rand(3, generator=torch.Generator().manual_seed(7)).to(cx.dev)
    stats = {"n": [], "jumped": 0}
    if loss_fn == "reference":
        loss_fn = lambda rgb, acc, depth, sem, pix, dep, lab: (F.smooth_l1_loss(rgb, pix) * 10 + F.smooth_l1_loss(depth, dep.unsqueeze(1)) / 5
                                                               + F.cross_entropy(sem, lab) / 2)

    def step(i):
        r, pix, dep_, lab = batches[i % 8]
        out = RD.train_step(tf, te, opt, r, pix, dep_, lab, bkd, step=1000 + i, sync=True, occ_thre=1e-2, loss_fn=loss_fn, **SC.RENDER_KW)
        stats["n"].append(out["n_rendering_samples"])
        stats["jumped"] += int(bool(out["skipped"]))
        return out
    return step, stats


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--rays", default="2000,8192")
    ap.add_argument("--only", default=None, help="run this leg alone: a, b, b+, b++ or c")
    ap.add_argument("--out", default=None, help="where the table goes (default: profiles/train_render_split.txt; nothing with --only)")
    a = ap.parse_args()
    assert a.reps >= 1 and a.steps >= 1
    if a.out is None and a.only is None:
        a.out = os.path.join(os.path.dirname(HERE), "profiles", "train_render_split.txt")
    cx = B.Ctx(B.parse(["--gpus", "1", "--workload", "train", "--warmup", "6", "--no-cpu-baseline"]))
    from apnrf_amd import render as RD
    tl = B.TrainLeg(cx, "102344280", seed=11)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# train render split: scene 102344280 (trained stand-in, every leg continued from its state), {a.reps} interleaved repetitions of {a.steps} steps after "
        f"warm-up; ms per step, median (min-max); device {cx.torch.cuda.get_device_name(0)}")
    say("# (a), (b) and (b+) start a fresh optimizer on the stand-in's parameters, (b++) and (c) continue the stand-in's Adam moments: the legs' sample counts drift "
        "apart over the repetitions (printed per leg). Read (a) against (b): same loop, same optimizer, the render alone swapped")
    for R_ in [int(x) for x in a.rays.split(",")]:
        legs = {
            "a": ("(a)   drop-in render + torch loss + isnan loop + torch Adam (the unchanged caller)",
                  lambda: reference_loop(cx, tl, R_, RD.render_image_with_occgrid_with_depth_guide)),
            "b": ("(b)   the same loop, fused_train_render swapped in",
                  lambda: reference_loop(cx, tl, R_, RD.fused_train_render)),
            "b+": ("(b+)  (b) with optim.FusedAdam bound to the field",
                   lambda: reference_loop(cx, tl, R_, RD.fused_train_render, fused_adam=True)),
            "b++": ("(b++) train_step(loss_fn=the reference's loss lines), FusedAdam",
                    lambda: train_step_leg(cx, tl, R_, "reference")),
            "c": ("(c)   train_step(fused=True), host-synchronous (the floor)",
                  lambda: train_step_leg(cx, tl, R_)),
        }
        if a.only is not None:
            legs = {a.only: legs[a.only]}
        made = {k: (label,) + make() for k, (label, make) in legs.items()}
        times = {k: [] for k in made}
        for rep in range(a.reps):
            for k, (label, step, stats) in made.items():
                times[k].append(1e3 * cx.timed(step, a.steps, 8 if rep == 0 else 2, False) / a.steps)
        say(f"## {R_} rays per step")
        for k, (label, step, stats) in made.items():
            t = times[k]
            say(f"{label:90s} {np.median(t):7.3f} ms ({min(t):.3f}-{max(t):.3f})  samples per step {np.mean(stats['n'][-a.steps:]):9.0f}  skipped {stats['jumped']}")
        if "a" in times and "b" in times:
            ta, tb = times["a"], times["b"]
            say(f"(a) - (b) = {np.median(ta) - np.median(tb):.3f} ms; (a)'s own min-max spread {max(ta) - min(ta):.3f} ms")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
