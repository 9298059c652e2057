"""GPU tests of the one-call train step (`render.fused_forward_backward`: `mnf_train_step`) and of the differentiable train render cut at its loss
(`render.fused_train_render`) away from the yaml's render options: cone angle 0 and no threshold (the reference functions' defaults), `early_stop_eps` 0 (no
filter at all: the ray-major density pre-pass never stops) and 0.2 (its cut at T < 0.1, visibility at 0.2), near and far planes that leave a quarter of the rays
empty, and an alpha threshold above `occs.mean()` (the mean decides, occ_grid.py:199).  `train_step` pins `far_plane` and `early_stop_eps`, so the options go
through the two entry points underneath it.

Reference: the oracle's autograd (`oracle.render.render_train`), bars of `_fused_step_vs_oracle` (tests/test_gpu_routes.py) and of tests/test_gpu_train_render.py.
Every case first asserts, on the CPU, that the oracle keeps the identical sample set under both accumulation orders of its matrix products
(`accum="k16_reversed"`): no sample of the case sits on a threshold, so the counts are compared exactly.

Sizes: 16 x 16 rays of pose 1; up to 25 000 kept samples (T1, T2), for which the oracle's autograd takes under a second."""
import numpy as np
import pytest
import torch

import helpers as H
from test_gpu_round6 import _check_grads, _loss
from test_gpu_routes import _fused_step_vs_oracle
from test_gpu_train_render import _check_planes

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

CASES = {
    "T1": dict(near_plane=0.0, render_step_size=5e-3, cone_angle=0.0, alpha_thre=0.0, early_stop_eps=1e-4),
    "T2": dict(near_plane=0.05, render_step_size=8e-3, cone_angle=0.0, alpha_thre=0.0, early_stop_eps=0.0),
    "T3": dict(H.RENDER_KW, alpha_thre=0.0, early_stop_eps=0.2),
    "T4": dict(near_plane=0.8, far_plane=3.0, render_step_size=2e-3, cone_angle=0.01, alpha_thre=0.05),
    "T5": dict(H.RENDER_KW, alpha_thre=0.5),
    "T6": dict(H.RENDER_KW, early_stop_eps=0.0),      # (not in the issue's table: what notices a pre-pass cut that ignores the option, see its test)
}
HW = {"T1": 16, "T2": 16, "T3": 16, "T4": 16, "T5": 16, "T6": 16}
POSE, SEED, LH = 1, 2, 14


def oracle_sampling(case, neurons=128, layers=2, C=29, precision="f16", accum="whole", occs_mean=None):
    """`oracle.render.sampling` of the case's batch (CPU only) -> (ray_indices, t_starts, t_ends, n_all)"""
    from apnrf_amd.nerfacc import OccGridEstimator
    from oracle import render as R
    sc = H.make_scene(neurons=neurons, layers=layers, C=C, log2_hashmap_size=LH, seed=SEED)
    orc = H.oracle_field(sc, precision=precision, accum=accum)
    o, d = H.view_rays(sc, POSE, h=HW[case], w=HW[case])
    kw = dict(CASES[case])
    near = torch.full((o.shape[0],), kw.pop("near_plane"))
    aabbs = OccGridEstimator(torch.from_numpy(sc["aabb"]), resolution=sc["res"], levels=1).aabbs.numpy()
    mean = float(torch.full((int(np.prod(sc["res"])),), 0.05).mean().item()) if occs_mean is None else occs_mean

    def sigma_fn(ts, te, ri):
        return orc.query_density(o[ri] + d[ri] * (ts + te)[:, None] / 2.0).squeeze(-1)
    return R.sampling(sc["occ"], aabbs, mean, o, d, sigma_fn, near, **kw)


def check_case_is_valid(case, **field):
    """Both accumulation orders keep the identical sample set.  A case that fails here is changed on the CPU, never given a budget."""
    a, b = oracle_sampling(case, accum="whole", **field), oracle_sampling(case, accum="k16_reversed", **field)
    n_rays = HW[case] ** 2
    empty = n_rays - int(np.count_nonzero(np.bincount(a[0].numpy(), minlength=n_rays)))
    print(f"{case} {field or ''}: marched {a[3]}, kept {len(a[0])}, rays with no sample {empty} of {n_rays}")
    assert a[3] == b[3] and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]), (case, len(a[0]), len(b[0]))
    return a, empty


def _case(case, neurons=128, layers=2, C=29, bf16=False):
    """The comparisons every case shares: the one-call step (`_fused_step_vs_oracle` with the case's options), then `fused_train_render` + the same loss
    in torch + backward on a fresh field against the same oracle render.  -> the step's result (with the oracle's render and the batch)"""
    from apnrf_amd import render as RD
    field_kw, oracle_kw = (dict(mfma_bf16=True), dict(precision="bf16")) if bf16 else (None, None)
    tol = 8.0 if bf16 else 1.0                                      # bf16: the value bars x 8, gradients at rel 6e-2 / cosine 0.998 (tests/test_gpu_precision_modes.py)
    bars = dict(loss_rtol=1e-4 * tol, rel=6e-2 if bf16 else 3e-2, cos=0.998 if bf16 else 0.999)
    ref_set, empty = check_case_is_valid(case, neurons=neurons, layers=layers, C=C, precision="bf16" if bf16 else "f16")
    out = _fused_step_vs_oracle(neurons, layers, C, LH, hw=HW[case], min_samples=1000, field_kw=field_kw, oracle_kw=oracle_kw, options=CASES[case],
                                scene_seed=SEED, pose=POSE, image=640, **bars)
    ref = out["ref"]
    assert torch.equal(ref[5]["t_starts"], ref_set[1]) and ref[5]["n_all"] == ref_set[3]      # the validity check looked at this very batch
    # the step cut at its loss
    hip2 = H.hip_field(out["sc"], **(field_kw or {})).train()
    pix, dep, lab = (t.to(DEV) for t in out["targets"])
    rgb, acc, depth, sem, n = RD.fused_train_render(hip2, out["est"], out["rays"], render_bkgd=out["bk"].to(DEV), stratified=False, **CASES[case])
    last = RD.latest_train_render(hip2)
    assert last is not None, "fused_train_render handed over"
    assert n == ref[4] and int(last["counts"][0]) == ref[5]["n_all"] and int(last["counts"][3]) == 0
    _check_planes((rgb, acc, depth, sem), ref, tol)
    loss = _loss(rgb, depth, sem, pix, dep, lab)
    loss.backward()
    print(f"{case} train render loss rel err {abs(float(loss) / float(out['ref_loss']) - 1.0):.2e}; against the one-call step {abs(float(loss) / float(out['loss']) - 1.0):.2e}")
    np.testing.assert_allclose(float(loss.detach()), float(out["ref_loss"]), rtol=bars["loss_rtol"])
    np.testing.assert_allclose(float(loss.detach()), float(out["loss"]), rtol=2e-5)
    _check_grads(hip2, out["orc"], rel=bars["rel"], cos=bars["cos"])
    out.update(planes=(rgb.detach(), acc.detach(), depth.detach(), sem.detach()), empty=empty)
    return out


@pytest.mark.parametrize("neurons,layers,C,bf16", [(128, 2, 29, False), (64, 4, 13, False), (128, 2, 29, True)])
def test_T1_reference_defaults_take_the_fused_route(neurons, layers, C, bf16):
    """near 0, cone 0, no threshold, eps 1e-4: the fused kernels themselves at the reference functions' defaults (tests/test_gpu_round6.py has these options only
    on a batch that hands over).  The route must be taken: no ray past the sampler's 2048-sample scratch row."""
    out = _case("T1", neurons, layers, C, bf16)
    assert 0 < int(out["counts"][2]) <= 2048, int(out["counts"][2])
    if neurons == 128:
        assert out["n_rendering_samples"] < 0.8 * out["n_marched"]      # eps 1e-4 alone filters (occ_grid.py:191); the 64 x 4 field of this seed is too thin for it


def test_T2_no_filter_at_all():
    """eps 0 and threshold 0: occ_grid.py:191's branch is skipped, every marched sample is kept, the pre-pass never stops a ray (`sdt_stop = INFINITY`)."""
    out = _case("T2")
    assert out["n_rendering_samples"] == out["n_marched"] == out["ref"][5]["n_all"]
    kw = dict(CASES["T2"]); kw.pop("early_stop_eps")
    ri, ts, te = out["est"].sampling(out["rays"].origins, out["rays"].viewdirs, sigma_fn=None, stratified=False, **kw)
    assert torch.equal(ts.cpu(), out["ref"][5]["t_starts"]) and torch.equal(te.cpu(), out["ref"][5]["t_ends"]) and torch.equal(ri.cpu(), out["ref"][5]["ray_indices"])


def test_T3_early_stop_eps_point_two():
    """eps 0.2: the pre-pass stops a ray at T < 0.1 (`sdt_stop = -log(0.2) + ln 2`), visibility is T >= 0.2: most marched samples go."""
    out = _case("T3")
    assert out["n_rendering_samples"] < 0.5 * out["n_marched"]


def test_T6_threshold_without_early_stop():
    """eps 0 with the yaml's alpha threshold: the filter runs (occ_grid.py:191) but nothing is ever invisible by transmittance, so the density pre-pass must walk
    every ray to its end (`sdt_stop = INFINITY`).  A cut placed where eps 1e-4 puts it (T < 5e-5) would leave zeros for the densities behind it, and the threshold
    would then drop samples the reference keeps; with a larger eps (T3) such a cut is merely late, and without a threshold (T2) the zeros are never looked at.  The
    oracle's record must show kept samples behind that point."""
    out = _case("T6")
    behind = int((out["ref"][5]["trans"] < 0.5e-4).sum())
    print(f"T6: kept samples with T < 5e-5: {behind}")
    assert behind >= 1000, behind


def test_T4_planes_leave_a_quarter_of_the_rays_empty():
    """near 0.8, far 3.0: `planes_kernel`, the far cut, and at least a quarter of the rays without a sample: background colour, zeros, and exactly no gradient
    of such a ray (`fused_train_render_rays`)."""
    from apnrf_amd import render as RD
    out = _case("T4")
    n_rays = HW["T4"] ** 2
    assert out["empty"] >= n_rays // 4, out["empty"]
    rgb, acc, depth, sem = out["planes"]
    none = torch.from_numpy(np.bincount(out["ref"][5]["ray_indices"].numpy(), minlength=n_rays) == 0).to(DEV)
    assert int(none.sum()) == out["empty"]
    assert torch.equal(rgb[none].cpu(), out["bk"].expand(out["empty"], 3)) and not acc[none].any() and not depth[none].any() and not sem[none].any()
    assert bool((acc[~none] > 0).all())
    hip3 = H.hip_field(out["sc"]).train()
    o, d = out["rays"].origins.clone().requires_grad_(True), out["rays"].viewdirs.clone().requires_grad_(True)
    pix, dep, lab = (t.to(DEV) for t in out["targets"])
    planes = RD.fused_train_render_rays(hip3, out["est"], RD.Rays(o, d), render_bkgd=out["bk"].to(DEV), stratified=False, **CASES["T4"])
    assert planes[4] == out["ref"][4]
    _loss(planes[0], planes[2], planes[3], pix, dep, lab).backward()
    assert not o.grad[none].any() and not d.grad[none].any()
    assert bool(torch.isfinite(o.grad).all()) and bool(torch.isfinite(d.grad).all()) and bool(d.grad[~none].any(1).all())


def test_T5_threshold_above_the_occupancy_mean():
    """alpha_thre 0.5 with `occs.mean()` 0.05: the threshold is the mean (`mean_final_kernel`; occ_grid.py:199).  With 0.5 itself the oracle keeps a different
    set, so the comparison tells the two apart."""
    out = _case("T5")
    other = oracle_sampling("T5", occs_mean=1.0)
    assert len(other[0]) < 0.9 * out["ref"][4], (len(other[0]), out["ref"][4])
