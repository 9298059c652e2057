"""Measurement of the held-out view evaluation (profiles/eval_views.txt): four 800 x 800 views at C = 29 of the bench
stand-in (scene 102344529).

  1. `mnf_eval_views` alone on the finished renders: time per call from the library's hipEvent pairs (`mnf_profile_begin/end`,
     label "eval_views": memset + both kernels), bytes read per pixel and the fraction of the 8 TB/s HBM figure, for both storage layouts.
  2. wall time of `render.evaluate_views` beside the same four images evaluated the way a caller had to before it existed:
     `ds[i]`, `render_image_with_occgrid_test`, the torch expressions of pipeline.py:588-605 with their `.item()` reads, and the
     `.cpu()` copies of the planes.  Same process, after warm-up, median of `--reps` repetitions.

    python tools/eval_views_measure.py [--reps 10] [--out FILE]
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
from apnrf_amd.dataset import Dataset  # noqa: E402

DEV = "cuda:0"
H = W = 800
C = 29
V = 4


def median_ms(fn, reps, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


def kernel_ms(lib, fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    lib.mnf_profile_begin()
    for _ in range(reps):
        fn()
    lib.mnf_profile_end(None, None)
    ms, n = ctypes.c_double(), ctypes.c_int64()
    lib.mnf_profile_query(b"eval_views", ctypes.byref(ms), ctypes.byref(n))
    return ms.value / max(n.value, 1), n.value


def reference_loop(field, est, ds, ids):
    """pipeline.py:553-613 without LPIPS, as a user of the import swap writes it."""
    psnrs, ces, deps = [], [], []
    for i in ids:
        data = ds[i]
        rgb, acc, depth, sem, _ = RD.render_image_with_occgrid_test(1024, field, est, data["rays"], render_bkgd=data["color_bkgd"], **SC.RENDER_KW)
        pixels, dep, sem_gt = data["pixels"], data["dep"], data["sem"]
        sem_gt.cpu().numpy(); sem.cpu().numpy()
        ces.append(F.cross_entropy(sem.reshape(-1, C), sem_gt.flatten()).item())
        mse = F.mse_loss(rgb, pixels)
        psnr = -10.0 * torch.log(mse) / np.log(10.0)
        psnrs.append(psnr.item())
        deps.append(F.mse_loss(depth, dep.unsqueeze(2)).item())
        pixels.cpu().numpy(); rgb.cpu().numpy(); dep.cpu().numpy(); depth.cpu().numpy()
        psnr.item()
    return np.mean(psnrs), np.mean(deps), np.mean(ces)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    lib = apnrf_amd.load_library()
    scene = SC.make_scene("102344529", n_poses=8)
    field, est, _ = ST.train_standin(scene, DEV)
    rng = np.random.default_rng(0)
    c2w = np.stack([RD.pose_to_c2w(np.asarray(p, np.float64)) for p in scene["poses"][:V]]).astype(np.float32)
    images = rng.integers(0, 256, size=(V, H, W, 3), dtype=np.uint8)
    depths = rng.uniform(0.2, 6.0, size=(V, H, W)).astype(np.float32)
    sems = rng.integers(0, C, size=(V, H, W)).astype(np.int64)
    sets = {}
    for name, packed in (("u8/f32/i64", False), ("u8/f16/u8 (packed)", True)):
        ds = Dataset(training=False, save_fp="", device=DEV, packed=packed)
        ds.update_data(images, depths, sems, c2w)
        sets[name] = ds
    ids = list(range(V))
    say(f"# held-out view evaluation: {V} views of {H}x{W}, C = {C}, trained stand-in of scene 102344529; medians of {a.reps} repetitions (min-max)")
    r = RD.evaluate_views(field, est, sets["u8/f32/i64"], ids, return_images=True, **SC.RENDER_KW)
    rgb, depth, sem = r["rgb"], r["depth"], r["sem"]
    for name, ds in sets.items():
        gt_bytes = 6 if ds.packed else 15
        per_pixel = (3 + 1 + C) * 4 + gt_bytes
        for conf, lab in ((True, False), (True, True), (False, False)):
            ms, n = kernel_ms(lib, lambda: RD.eval_metrics(rgb, depth, sem, ds, ids, confusion=conf, labels=lab), 20)
            tbs = per_pixel * V * H * W / (ms * 1e-3) / 1e12
            say(f"mnf_eval_views  {name:20s} confusion={int(conf)} labels={int(lab)}: {1e3 * ms:8.1f} us per call ({n} calls, hipEvents), "
                f"{per_pixel} B read per pixel -> {tbs:.2f} TB/s = {tbs / 8.0:.3f} of 8 TB/s")
    for name, ds in sets.items():
        fused = median_ms(lambda: RD.evaluate_views(field, est, ds, ids, views_per_call=4, **SC.RENDER_KW), a.reps)
        one = median_ms(lambda: RD.evaluate_views(field, est, ds, ids, views_per_call=1, **SC.RENDER_KW), a.reps)
        loop = median_ms(lambda: reference_loop(field, est, ds, ids), a.reps)
        say(f"wall  {name:20s} evaluate_views(views_per_call=4) {fused[0]:7.1f} ms ({fused[1]:.1f}-{fused[2]:.1f}) | views_per_call=1 {one[0]:7.1f} ms "
            f"({one[1]:.1f}-{one[2]:.1f}) | per-image loop with torch metrics and host copies {loop[0]:7.1f} ms ({loop[1]:.1f}-{loop[2]:.1f}) "
            f"-> {loop[0] / fused[0]:.2f}x")
    rays = [sets["u8/f32/i64"][i]["rays"] for i in ids]
    o, d = torch.cat([x.origins.reshape(-1, 3) for x in rays]), torch.cat([x.viewdirs.reshape(-1, 3) for x in rays])
    render_only = median_ms(lambda: RD.render_views(field, est, o, d, H * W, image_hw=(H, W), render_bkgd=torch.ones(3), n_split=None, **SC.RENDER_KW),
                            a.reps)
    say(f"wall  the four renders alone (one batched call, rays resident)   {render_only[0]:7.1f} ms ({render_only[1]:.1f}-{render_only[2]:.1f})")
    ev = RD.evaluate_views(field, est, sets["u8/f32/i64"], ids, **SC.RENDER_KW)
    lp = reference_loop(field, est, sets["u8/f32/i64"], ids)
    say(f"values  evaluate_views mean: {ev['mean']}  | loop (fp32 torch): psnr {lp[0]:.6f} depth_mse {lp[1]:.6f} sem_ce {lp[2]:.6f}")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
