"""Render tiles without a kept sample stop behind the density (csrc/field.hip, `dead_tile_rays` in csrc/composite_dev.h): the reference drops every sample with
alpha < alpha_thre before it accumulates anything (utils.py:714-725), so a 64-column tile in which no sample passes needs neither the heads nor the compositing, only
the retirement of its rays.

The helpers' random-weight scene has no such tile (median density 17 /m: alpha ~ 0.017 per step, every sample counts), so the density-logit row of its base MLP is
scaled by 0.2 here: alpha then grows with the distance (dt = 0.004 t) through the threshold, the samples near the camera are invisible together and the rounds mix
dead and live tiles in every slot form.  Chosen on the CPU with the oracle: kept samples counted per 64-column group of every round of the rays below (40 x 40 rays,
reference schedule, 42 rounds: 17 of the first round's 100 groups have none, 1..7 of the 20..30 groups of the rounds with strides 5 .. 18)."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import helpers as H

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DENSITY_ROW_SCALE = 0.2


def scale_density_row(scene, factor):
    """the density-logit row (row 0) of the base MLP's output layer, in place; factor 0 zeroes the WHOLE output layer (logit 0, geo features 0)"""
    W, layers = scene["neurons"], scene["layers"]
    off = W * 64 + (layers - 1) * W * W
    if factor == 0:
        scene["params"]["mlp_base"][off:off + 16 * W] = 0.0
    else:
        scene["params"]["mlp_base"][off:off + W] *= np.float32(factor)
    return scene


def test_dead_tiles_skip_heads_and_compositing_without_moving_a_bit():
    """Skip on against skip off (MNF_NO_TILE_SKIP=1, read by the diagnostic library only) on the same rays and schedules: every output bit for bit, and the round
    log shows rounds with dead and live tiles.  Child process on libmi355nerf_diag.so (tests/diag_tile_skip.py)."""
    from apnrf_amd import build as B
    here = os.path.dirname(os.path.abspath(__file__))
    assert os.path.exists(B.LIB_DIAG), "libmi355nerf_diag.so missing: run `python __graft_entry__.py build`"
    env = dict(os.environ, MNF_LIB_PATH=B.LIB_DIAG)
    r = subprocess.run([sys.executable, os.path.join(here, "diag_tile_skip.py")], env=env, capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and "DIAG_TILE_SKIP_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


class _InvisibleField:
    """What the oracle's field answers once the base MLP's output layer is zero: logit 0, density exp(-1) inside the box (ngp.py:79, :179, :193-195) and 0 outside;
    colours and logits never count (no sample passes the threshold).  Counts the samples it is asked for: the oracle's marched total."""

    def __init__(self, scene, real):
        self.num_semantic_classes = real.num_semantic_classes
        self.real, self.aabb, self.marched, self.checked = real, torch.from_numpy(scene["aabb"]), 0, 0

    def __call__(self, pos, dirs):
        self.marched += pos.shape[0]
        xn = (pos - self.aabb[:3]) / (self.aabb[3:] - self.aabb[:3])
        inside = ((xn > 0) & (xn < 1)).all(-1)
        sigma = torch.where(inside, torch.tensor(math.exp(-1.0), dtype=torch.float32), torch.tensor(0.0))
        if self.checked < 2 and pos.shape[0]:                      # the stand-in IS the oracle's field on these weights (spot check: the full field on 200 000 samples takes minutes)
            self.checked += 1
            assert torch.equal(self.real(pos[:512], dirs[:512])[1].squeeze(-1), sigma[:512])
        return torch.zeros(pos.shape[0], 3), sigma[:, None], torch.zeros(pos.shape[0], self.num_semantic_classes)


def _diag_rays(scene):
    oa, da = H.view_rays(scene, 2, h=48, w=48)
    ob, db = H.view_rays(scene, 5, h=48, w=48)
    return torch.cat([oa, ob, oa[:150]]), torch.cat([da, db, da[:150]])      # two views and a ragged rest, as tests/diag_tile_skip.py


def test_all_tiles_dead_known_answer():
    """Base MLP output layer zeroed: logit 0, sigma = exp(-1), alpha = 1 - exp(-sigma dt) with dt = max(1e-3, 0.004 t).  alpha stays below the 0.01 threshold only
    up to t = 6.8 m (the scene box is 19 m long: with the default far plane the oracle keeps 18 854 samples of these rays), so the far plane is put at 6 m: then
    alpha <= 8.8e-3 at every sample, every tile is dead and the answer is known exactly: background colour, zero everywhere else, no kept sample.  The evaluated
    total pins the dead path's ray retirement: a ray kept alive or retired wrongly changes the later budgets and with them the count (oracle: 197 394 samples in
    21 rounds, strides 4 .. 64)."""
    from apnrf_amd import render as RD
    from oracle import render as R
    sc = scale_density_row(H.make_scene(), 0)
    hip, est = H.hip_field(sc), H.hip_estimator(sc)
    o, d = _diag_rays(sc)
    n = o.shape[0]
    bk = torch.tensor([0.1, 0.3, 0.6])
    counting = _InvisibleField(sc, H.oracle_field(sc))
    ref = R.render_test(1024, counting, sc["occ"], sc["aabb"][None], o, d, render_bkgd=bk, far_plane=6.0, **H.RENDER_KW)
    assert ref["total_samples"] == 0 and counting.marched > 30 * n and len({s for _, s in ref["rounds"]} - {4, 8, 16}) > 2
    for prob in (False, True):
        out = RD.render_views(hip, est, o.to(DEV), d.to(DEV), n, 1024, render_bkgd=bk, far_plane=6.0, probabilistic=prob, **H.RENDER_KW)
        assert torch.equal(out["rgb"].cpu(), bk.expand(n, 3))
        for k in ("acc", "depth", "sem") + (("rgb_var", "depth_var") if prob else ()):
            assert not out[k].any(), k
        assert int(out["total"][0]) == 0
        assert int(out["total"][1]) == counting.marched, (int(out["total"][1]), counting.marched)


@pytest.fixture(scope="module")
def mixed():
    sc = scale_density_row(H.make_scene(), DENSITY_ROW_SCALE)
    o, d = H.view_rays(sc, 2, h=32, w=32)
    return sc, H.hip_field(sc), H.hip_estimator(sc), H.oracle_field(sc), o, d


@pytest.mark.parametrize("prob", [False, True])
def test_mixed_tiles_match_oracle(mixed, prob, monkeypatch):
    """Oracle parity where dead and live tiles mix, with the bars of the existing render tests: rgb / acc / depth (and the variances, test_gpu_parity._check_render)
    within 1e-3 absolute, class logits within max(1e-3, 3e-4 x the ray's largest |logit|) (tests/test_gpu_round4.py), at most 2 rays outside on an alpha-threshold tie
    and those within 5e-2, kept totals within max(3, 0.2 %).  The product library reads no knob: the same render with the diagnostic variables set keeps its bits."""
    from apnrf_amd import render as RD
    from oracle import render as R
    sc, hip, est, orc, o, d = mixed
    n = o.shape[0]
    bk = torch.tensor([0.1, 0.3, 0.6])
    ref = (R.render_prob_test if prob else R.render_test)(1024, orc, sc["occ"], sc["aabb"][None], o, d, render_bkgd=bk, **H.RENDER_KW)
    assert len(ref["rounds"]) > 20 and 0.2 * n < ref["total_samples"]
    out = RD.render_views(hip, est, o.to(DEV), d.to(DEV), n, 1024, render_bkgd=bk, probabilistic=prob, **H.RENDER_KW)
    assert int(out["total"][0]) < 0.6 * int(out["total"][1])                        # a good part of the evaluated samples is invisible
    sem_bar = np.maximum(1e-3, 3e-4 * ref["sem"].abs().max(dim=1, keepdim=True).values.numpy())
    keys = [("rgb", 1e-3, 0.0), ("acc", 1e-3, 0.0), ("depth", 1e-3, 1e-3), ("sem", sem_bar, 0.0)]
    if prob:
        keys += [("rgb_var", 1e-3, 0.0), ("depth_var", 2e-3, 2e-3)]
    bad = np.zeros(n, bool)
    for k, atol, rtol in keys:
        got, want = out[k].cpu().numpy().reshape(n, -1), ref[k].numpy().reshape(n, -1)
        err = np.abs(got - want)
        print(f"prob {prob} {k}: max |error| {err.max():.3e}")
        bad |= (err > atol + rtol * np.abs(want)).any(1)
        np.testing.assert_allclose(got, want, atol=5e-2, rtol=5e-2, err_msg=k)
    print(f"prob {prob}: rays outside the bars {int(bad.sum())}, kept {int(out['total'][0])} vs oracle {ref['total_samples']}, evaluated {int(out['total'][1])}")
    assert bad.sum() <= 2, int(bad.sum())
    assert abs(int(out["total"][0]) - ref["total_samples"]) <= max(3, 0.002 * ref["total_samples"])
    for name in ("MNF_NO_TILE_SKIP", "MNF_TILE_SKIP_ALL"):
        monkeypatch.setenv(name, "1")
    again = RD.render_views(hip, est, o.to(DEV), d.to(DEV), n, 1024, render_bkgd=bk, probabilistic=prob, **H.RENDER_KW)
    for k in out:
        assert torch.equal(out[k], again[k]), k
