"""Measurement of the structural-similarity pass (profiles/ssim_views.txt): four 800 x 800 views of the bench stand-in
(scene 102344529), one process, after warm-up.

  1. `mnf_ssim_views` alone on the finished rgb renders: time per call from the library's hipEvent pairs (`mnf_profile_begin/end`, label
     "ssim_views": both kernels), against its algorithmic bytes (4 K read of the render + K read of the u8 target per pixel; + 8 written
     per window centre with the map), for the u8 and the f32 target, with and without the map.
  2. wall time of three legs, interleaved (a, b, c, a, b, c, ...), median and min-max of `--reps` repetitions each:
       (a) `evaluate_views(ssim=False)`;
       (b) `evaluate_views(ssim=True)`;
       (c) the caller's way before `ssim=True` existed: `evaluate_views(return_images=True)`, the rgb planes copied to the host with
           `.cpu()`, and the 11 x 11 Gaussian filter there (`scipy.ndimage.gaussian_filter` in float64 as skimage runs it when scipy is
           importable, else the numpy restatement of tests/ssim_ref.py).

    python tools/ssim_measure.py [--reps 10] [--out FILE]
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
sys.path.insert(0, os.path.join(REPO, "tests"))
import apnrf_amd  # noqa: E402
import ssim_ref as SR  # noqa: E402
from apnrf_amd import render as RD  # noqa: E402
from apnrf_amd import scenes as SC  # noqa: E402
from apnrf_amd import standin as ST  # noqa: E402
from apnrf_amd.dataset import Dataset  # noqa: E402

try:
    from scipy import ndimage as ndi
except ImportError:
    ndi = None

DEV = "cuda:0"
H = W = 800
C = 29
V = 4
K = 3


def kernel_ms(lib, fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    lib.mnf_profile_begin()
    for _ in range(reps):
        fn()
    lib.mnf_profile_end(None, None)
    ms, n = ctypes.c_double(), ctypes.c_int64()
    lib.mnf_profile_query(b"ssim_views", ctypes.byref(ms), ctypes.byref(n))
    return ms.value / max(n.value, 1), n.value


def host_ssim(x, y):
    """Per-view SSIM of [V,H,W,3] fp32 host arrays, as skimage computes it (float64, gaussian_weights=True, sigma=1.5, crop 5)."""
    if ndi is None:
        return SR.ssim(x, y)[0]
    x, y = x.astype(np.float64), y.astype(np.float64)
    c1, c2 = SR.K1 ** 2, SR.K2 ** 2
    f = lambda a: ndi.gaussian_filter(a, sigma=(0, SR.SIGMA, SR.SIGMA, 0), truncate=3.5, mode="reflect")
    ux, uy = f(x), f(y)
    vx, vy, vxy = f(x * x) - ux * ux, f(y * y) - uy * uy, f(x * y) - ux * uy
    s = ((2 * ux * uy + c1) * (2 * vxy + c2)) / ((ux * ux + uy * uy + c1) * (vx + vy + c2))
    return s[:, 5:-5, 5:-5].reshape(x.shape[0], -1).mean(axis=1)


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
    ds = Dataset(training=False, save_fp="", device=DEV)
    ids = list(range(V))
    ds.update_data(np.zeros((V, H, W, 3), np.uint8), rng.uniform(0.2, 6.0, size=(V, H, W)).astype(np.float32),
                   rng.integers(0, C, size=(V, H, W)).astype(np.int64), c2w)
    # ground-truth images that resemble the renders (the renders themselves plus noise, stored as u8): SSIM in the range a trained model gives
    r = RD.evaluate_views(field, est, ds, ids, return_images=True, **SC.RENDER_KW)
    noisy = (r["rgb"].cpu().numpy() + 0.05 * rng.standard_normal((V, H, W, 3))).clip(0, 1)
    ds.images = torch.from_numpy(np.rint(noisy * 255).astype(np.uint8)).to(DEV)
    rgb = r["rgb"]
    pixels = torch.stack([ds[i]["pixels"] for i in ids])
    say(f"# structural similarity: {V} views of {H}x{W}x{K}, trained stand-in of scene 102344529; host filter: "
        f"{'scipy.ndimage.gaussian_filter' if ndi is not None else 'numpy restatement'}")

    centres = (H - 10) * (W - 10)
    for name, fn, rd in (("u8 target ", lambda m: RD.ssim_metrics(rgb, ds, ids, maps=m), 4 * K + K),
                         ("f32 target", lambda m: RD.ssim_views(rgb, pixels, maps=m), 8 * K)):
        for m in (False, True):
            ms, n = kernel_ms(lib, lambda: fn(m), 20)
            nbytes = V * (rd * H * W + (8 * centres if m else 0))
            say(f"mnf_ssim_views  {name} map={int(m)}: {1e3 * ms:8.1f} us per call ({n} calls, hipEvents), {rd} B read per pixel"
                f"{' + 8 B written per centre' if m else ''} = {nbytes / 1e6:.1f} MB -> {nbytes / (ms * 1e-3) / 1e12:.3f} TB/s = "
                f"{nbytes / (ms * 1e-3) / 8e12:.4f} of 8 TB/s; {1e6 * ms / (V * centres * K):.3f} ns per centre and channel")

    def leg_a():
        return RD.evaluate_views(field, est, ds, ids, **SC.RENDER_KW)

    def leg_b():
        return RD.evaluate_views(field, est, ds, ids, ssim=True, **SC.RENDER_KW)

    def leg_c():
        out = RD.evaluate_views(field, est, ds, ids, return_images=True, **SC.RENDER_KW)
        out["ssim"] = host_ssim(out["rgb"].cpu().numpy(), np.stack([ds[i]["pixels"].cpu().numpy() for i in ids]))
        return out

    legs = (("(a) evaluate_views(ssim=False)", leg_a), ("(b) evaluate_views(ssim=True)", leg_b),
            ("(c) return_images=True, .cpu(), host filter", leg_c))
    for _, fn in legs:                                            # warm-up
        fn()
    torch.cuda.synchronize()
    ts = {name: [] for name, _ in legs}
    for _ in range(a.reps):
        for name, fn in legs:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts[name].append(1e3 * (time.perf_counter() - t0))
    say(f"# wall time, legs interleaved, {a.reps} repetitions each: median (min-max)")
    for name, _ in legs:
        t = np.asarray(ts[name])
        say(f"wall  {name:48s} {np.median(t):8.1f} ms ({t.min():.1f}-{t.max():.1f})")
    b, c = leg_b(), leg_c()
    say(f"values  device ssim {b['ssim'].tolist()}  host ssim {np.asarray(c['ssim']).tolist()}  max abs diff {np.abs(b['ssim'] - c['ssim']).max():.3e}")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
