"""GPU parity tests for the field's precision switches (`mnf_field_config`, include/mi355nerf.h): `mfma_bf16` (bf16 matrix-core operands, a second
translation unit of field.hip / train.hip), `blend_fp16` (tiny-cuda-nn's fp16 hash blend, the B16 instantiations, no feature rows in the train step) and
`output_fp16` (every network output handed over in fp16).  Each mode is compared with the oracle configured with the SAME mode — forward and density-only,
autograd backward, fused train step, fused test render, density pre-pass, presampled steps — at the bars of the default-mode test it mirrors (bf16: 8x the
fp16 bars, gradients 6e-2 relative L2 with cosine > 0.998).  Every case also proves that its switch is on: the same route with the switch flipped gives
different bits."""
import numpy as np
import pytest
import torch

import helpers as H
from test_gpu_parity import _check_render, _grad_close
from test_gpu_routes import _backward_vs_oracle, _cu, _fused_step_vs_oracle

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _mode(bf16=False, blend=False, out16=False):
    """-> (hip_field keywords, oracle_field keywords) of one precision mode"""
    field_kw = dict(mfma_bf16=bf16, tcnn_blend_fp16=blend, tcnn_output_rounding=out16)
    oracle_kw = dict(precision="bf16" if bf16 else "f16", blend="f16" if blend else "f32", output_rounding=out16)
    return field_kw, oracle_kw


def _flip(field_kw, key):
    return dict(field_kw, **{key: not field_kw[key]})


# ------------------------------------------------------------------ a. forward and density-only
def _forward_case(neurons, layers, C, lh, bf16=False, blend=False, out16=False):
    """test_field_forward_matches_oracle's comparison in one mode (bars x8 in bf16); returns the inputs and outputs for further checks"""
    field_kw, oracle_kw = _mode(bf16, blend, out16)
    sc = H.make_scene(neurons=neurons, layers=layers, C=C, log2_hashmap_size=lh, head_gain=4.0)
    hip, orc = H.hip_field(sc, **field_kw), H.oracle_field(sc, **oracle_kw)
    rng = np.random.default_rng(1)
    n = 5000 + 37                                                  # ragged tail (not a multiple of 64)
    a = sc["aabb"]
    pos = (rng.random((n, 3)) * (a[3:] - a[:3]) * 1.1 + a[:3] - 0.05 * (a[3:] - a[:3])).astype(np.float32)   # some outside the box
    d = rng.normal(size=(n, 3)).astype(np.float32); d /= np.linalg.norm(d, axis=-1, keepdims=True)
    with torch.no_grad():
        rgb, sigma, sem = hip(_cu(pos), _cu(d))
        dens = hip.query_density(_cu(pos))
    r_rgb, r_sigma, r_sem = orc(torch.from_numpy(pos), torch.from_numpy(d))
    assert sem.shape == (n, C) and rgb.shape == (n, 3) and sigma.shape == (n, 1)
    inside = (r_sigma[:, 0] > 0).numpy()
    sg, rsg = sigma.cpu().numpy(), r_sigma.numpy()
    print(f"forward {neurons}x{layers} C={C} {field_kw}: rgb max abs {np.abs(rgb.cpu().numpy() - r_rgb.numpy())[inside].max():.2e}, sigma max rel "
          f"{(np.abs(sg - rsg) / (rsg + 1e-6)).max():.2e}, sem max err / (1 + |logit|) "
          f"{(np.abs(sem.cpu().numpy() - r_sem.numpy()) / (1.0 + np.abs(r_sem.numpy())))[inside].max():.2e}")
    assert (sg[:, 0] > 0).tolist() == inside.tolist()                            # selector mask is exact
    np.testing.assert_array_equal(dens.cpu().numpy(), sg)                        # density-only kernel == full kernel, in this mode
    tol = 8.0 if bf16 else 1.0
    if out16 and not bf16:
        # test_field_tcnn_output_rounding_matches_oracle's bar: a logit whose fp32 pre-image sits within the summation-order difference of an fp16
        # rounding boundary moves by one fp16 ulp (2^-8 relative at |logit| in [4, 8))
        np.testing.assert_allclose(sg, rsg, rtol=9e-3, atol=1e-6)
        assert (np.abs(sg - rsg) > 2e-3 * np.abs(rsg) + 1e-6).mean() < 5e-3
    else:
        np.testing.assert_allclose(sg, rsg, rtol=2e-3 * tol, atol=1e-6)
    np.testing.assert_allclose(rgb.cpu().numpy()[inside], r_rgb.numpy()[inside], atol=1e-3 * tol, rtol=0)
    np.testing.assert_allclose(sem.cpu().numpy()[inside], r_sem.numpy()[inside], atol=1e-3 * tol, rtol=2e-3 * tol)
    assert np.abs(r_sem.numpy()).max() > 0.3                                     # the comparison is not vacuous
    return sc, field_kw, pos, d, (rgb, sigma, sem)


def _differs(sc, field_kw, pos, d, outs):
    """the same forward with `field_kw` (one switch flipped) gives other bits"""
    with torch.no_grad():
        other = H.hip_field(sc, **field_kw)(_cu(pos), _cu(d))
    assert not torch.equal(other[2], outs[2]) and not torch.equal(other[1], outs[1]), f"switch has no effect: {field_kw}"


SHAPES_AT_PADDING_EDGES = [(128, 1, 1, 12), (128, 2, 16, 15), (128, 3, 17, 19), (128, 4, 32, 12),
                           (64, 1, 17, 15), (64, 2, 32, 19), (64, 3, 16, 12), (64, 4, 1, 19)]


@pytest.mark.parametrize("neurons,layers,C,lh", SHAPES_AT_PADDING_EDGES[:-1] + [(64, 4, 29, 19)])
def test_bf16_forward_every_shape(neurons, layers, C, lh):
    """Every (neurons, layers) instantiation of the bf16 unit's field kernel (full and density-only), C at the head's padding edges (1, 16, 17, 32).
    64 x 4 runs with config 2's 29 classes: its single class logit stays below the 0.3 that makes the comparison non-vacuous (max 0.21)."""
    sc, kw, pos, d, outs = _forward_case(neurons, layers, C, lh, bf16=True)
    _differs(sc, _flip(kw, "mfma_bf16"), pos, d, outs)


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("layers,C,lh", [(1, 17, 12), (2, 29, 15), (3, 1, 14), (4, 32, 12)])
def test_blend_fp16_forward_every_128_shape(layers, C, lh, bf16):
    """The B16 instantiations (neurons = 128 only) of both units against the oracle's fp16 blend."""
    sc, kw, pos, d, outs = _forward_case(128, layers, C, lh, bf16=bf16, blend=True)
    _differs(sc, _flip(kw, "tcnn_blend_fp16"), pos, d, outs)


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("neurons,layers,C,lh", [(128, 2, 29, 14), (64, 4, 17, 12)])
def test_output_fp16_forward(neurons, layers, C, lh, bf16):
    """`output_fp16` in both units: the outputs are fp16 values, and they are the fp16 rounding of what the same unit computes with the flag off.
    The density logit (base network output) is rounded before anything else sees it, so log(sigma) moves by at most half an fp16 ulp of the logit
    (2^-11 relative) against the flag-off kernel.  In the fp16 unit the heads then see the same operands (an fp16 geometry feature is its own
    rounding), so the class logits move by at most half an fp16 ulp too; in the bf16 unit the heads see bf16(fp16(feature)) instead of bf16(feature),
    so only their grain is checked: fp16's 11 significand bits, not bf16's 8."""
    sc, kw, pos, d, outs = _forward_case(neurons, layers, C, lh, bf16=bf16, out16=True)
    with torch.no_grad():
        off = H.hip_field(sc, **_flip(kw, "tcnn_output_rounding"))(_cu(pos), _cu(d))
    _, sigma, sem = (t.cpu().numpy().astype(np.float64) for t in outs)
    _, sigma0, sem0 = (t.cpu().numpy().astype(np.float64) for t in off)
    inside = sigma0[:, 0] > 0
    logit0 = np.log(sigma0[inside, 0]) + 1.0
    dlog = np.abs(np.log(sigma[inside, 0]) - np.log(sigma0[inside, 0]))
    print(f"output_fp16 {neurons}x{layers} bf16={bf16}: |d log sigma| / |logit| max {(dlog / np.maximum(np.abs(logit0), 1e-30)).max():.3e} "
          f"(half an fp16 ulp: {2 ** -11:.3e})")
    assert (dlog <= 2 ** -11 * 1.01 * np.abs(logit0) + 2e-6).all(), float((dlog / np.maximum(np.abs(logit0), 1e-30)).max())
    s = outs[2].cpu().numpy()
    np.testing.assert_array_equal(s, s.astype(np.float16).astype(np.float32))           # the class logits are fp16 values ...
    grain = float((s != torch.from_numpy(s).bfloat16().float().numpy()).mean())
    print(f"output_fp16 {neurons}x{layers} bf16={bf16}: class logits that are not bf16 values {grain:.3f}")
    assert grain > 0.5                                                                   # ... with fp16's grain, not bf16's
    if not bf16:
        np.testing.assert_allclose(sem, sem0, rtol=2 ** -11 * 1.01, atol=1e-7)
    assert not torch.equal(outs[2], off[2])


# ------------------------------------------------------------------ b. backward through the autograd route
BF16 = dict(field_kw=_mode(bf16=True)[0], oracle_kw=_mode(bf16=True)[1], rel=6e-2, cos=0.998, fwd_atol=8e-3)


@pytest.mark.parametrize("neurons,layers,C,lh", SHAPES_AT_PADDING_EDGES)
def test_bf16_backward_every_shape(neurons, layers, C, lh):
    """test_field_backward_every_shape in the bf16 unit: every dgrad / wgrad instantiation, the semantic output layer class by class, padding rows zero."""
    _backward_vs_oracle(neurons, layers, C, lh, n=3000 + 21, seed=7, flip_kw=_flip(BF16["field_kw"], "mfma_bf16"), **BF16)


@pytest.mark.parametrize("lh,n", [(12, 8191), (12, 8192), (21, 12000), (22, 12000)])
def test_bf16_backward_scatter_routes(lh, n):
    """test_field_backward_scatter_routes in the bf16 unit: one bin per level on either side of n = 8192, 512 bins (the limit), walk only; level by level."""
    hip, orc, n_mlp = _backward_vs_oracle(128, 2, 29, lh, n=n, seed=17 + lh, **BF16)
    _, _, size, off, hashed = hip.grid_meta()
    assert sum(size) * 4 == orc.p_base.grad.numel() - n_mlp
    got = hip.mlp_base.params.grad[n_mlp:].view(-1, 4)
    want = orc.p_base.grad[n_mlp:].view(-1, 4)
    for lvl in range(16):
        sl = slice(off[lvl], off[lvl] + size[lvl])
        _grad_close(got[sl], want[sl], f"table level {lvl} ({size[lvl]} entries, hashed={hashed[lvl]})", rel=6e-2, cos=0.998)


@pytest.mark.parametrize("bf16", [False, True])
def test_blend_fp16_backward(bf16):
    """The B16 train forward and its backward against the oracle's fp16 blend (straight-through gradient of the half-precision sum)."""
    field_kw, oracle_kw = _mode(bf16=bf16, blend=True)
    bars = dict(rel=6e-2, cos=0.998, fwd_atol=8e-3) if bf16 else {}
    _backward_vs_oracle(128, 2, 29, 14, n=3000 + 21, seed=7, field_kw=field_kw, oracle_kw=oracle_kw, flip_kw=_flip(field_kw, "tcnn_blend_fp16"), **bars)


# ------------------------------------------------------------------ c. fused train step against oracle autograd
def test_bf16_fused_step_config5_model_binned():
    """BASELINE config 5's model (128 x 2, 29 classes, T = 2^19) in the bf16 unit: the feature-row route of the fused step, with >= 8192 samples so that
    the fine levels go through the binned scatter."""
    kw, okw = _mode(bf16=True)
    _fused_step_vs_oracle(128, 2, 29, 19, hw=32, min_samples=8192, field_kw=kw, oracle_kw=okw, loss_rtol=8e-4, rel=6e-2, cos=0.998,
                          flip_kw=_flip(kw, "mfma_bf16"))


def test_bf16_fused_step_64x4():
    """64 x 4, 29 classes in the bf16 unit: no feature rows (neurons != 128)."""
    kw, okw = _mode(bf16=True)
    _fused_step_vs_oracle(64, 4, 29, 15, hw=20, min_samples=2000, field_kw=kw, oracle_kw=okw, loss_rtol=8e-4, rel=6e-2, cos=0.998,
                          flip_kw=_flip(kw, "mfma_bf16"))


@pytest.mark.parametrize("bf16", [False, True])
def test_blend_fp16_fused_step_takes_the_rowless_route(bf16):
    """The fused step with tcnn's fp16 blend: `field_rows_supported` is false, so the step gathers from the table twice instead of keeping feature rows.
    The workspace proves it: smaller than the default field's of the same shape by exactly the rows ([max_marched][64] x 16 bit) and `k_src`
    ([max_kept] x int64), each rounded up to 256 bytes."""
    from apnrf_amd import _lib as L
    kw, okw = _mode(bf16=bf16, blend=True)
    bars = dict(loss_rtol=8e-4, rel=6e-2, cos=0.998) if bf16 else {}
    _fused_step_vs_oracle(128, 2, 29, 15, hw=20, min_samples=2000, field_kw=kw, oracle_kw=okw, flip_kw=_flip(kw, "tcnn_blend_fp16"), **bars)
    lib = L.load_library()
    sc = H.make_scene(neurons=128, layers=2, C=29, log2_hashmap_size=15)
    blend_f, plain_f = H.hip_field(sc, **kw), H.hip_field(sc, **_flip(kw, "tcnn_blend_fp16"))
    R, cap_m, cap_k = 1000, 100003, 50001
    up = lambda b: (b + 255) // 256 * 256
    nb = int(lib.mnf_train_step_workspace_bytes(blend_f._ensure_handle(), R, cap_m, cap_k))
    npl = int(lib.mnf_train_step_workspace_bytes(plain_f._ensure_handle(), R, cap_m, cap_k))
    assert nb > 0 and npl - nb == up(cap_m * 128) + up(cap_k * 8), (npl, nb)


def test_output_fp16_fused_step():
    """The fused step with every network output handed over in fp16 (the train forward rounds as the inference kernel does) against the tcnn oracle."""
    kw, okw = _mode(out16=True)
    _fused_step_vs_oracle(128, 2, 29, 15, hw=20, min_samples=2000, field_kw=kw, oracle_kw=okw, flip_kw=_flip(kw, "tcnn_output_rounding"))


# ------------------------------------------------------------------ d. fused test render
def _check_render_bf16(out, ref, prob, max_tie_rays=3):
    """_check_render's keys at 8x its bars (bf16 keeps 8 significand bits); a few alpha-threshold ties at bf16 resolution, PSNR > 40 dB as in
    test_bf16_field_forward_backward_and_render_match_oracle"""
    keys = [("rgb", 8e-3, 0.0), ("acc", 8e-3, 0.0), ("depth", 8e-3, 8e-3), ("sem", 8e-3, 0.0)]
    if prob:
        keys += [("rgb_var", 8e-3, 0.0), ("depth_var", 1.6e-2, 1.6e-2)]
    bad = np.zeros(ref["rgb"].shape[0], bool)
    for k, atol, rtol in keys:
        got, want = out[k].cpu().numpy(), ref[k].numpy()
        assert np.isfinite(got).all(), k
        viol = np.abs(got - want) > atol + rtol * np.abs(want)
        bad |= viol.reshape(viol.shape[0], -1).any(1)
    mse = float(((out["rgb"].cpu() - ref["rgb"]) ** 2).mean())
    tot = int(out["total"][0].item())
    print(f"bf16 render prob={prob}: rays outside 8x the fp16 bars {int(bad.sum())}, PSNR vs oracle {10.0 * np.log10(1.0 / max(mse, 1e-20)):.1f} dB, "
          f"samples {tot} vs {ref['total_samples']}")
    assert bad.sum() <= max_tie_rays, f"{bad.sum()} rays outside 8x the fp16 bars"
    assert 10.0 * np.log10(1.0 / max(mse, 1e-20)) > 40.0
    assert abs(tot - ref["total_samples"]) <= max(3, 0.002 * ref["total_samples"]), (tot, ref["total_samples"])


def _render_case(sc, pose, hw, width, bk, kw, okw, flip_key, prob, check):
    from apnrf_amd import render as RD
    from oracle import render as R
    hip, orc, est = H.hip_field(sc, **kw), H.oracle_field(sc, **okw), H.hip_estimator(sc)
    o, d = H.view_rays(sc, pose, width=width, height=width, h=hw, w=hw)
    fn = R.render_prob_test if prob else R.render_test
    ref = fn(1024, orc, sc["occ"], sc["aabb"][None], o, d, render_bkgd=bk, **H.RENDER_KW)
    out = RD.render_views(hip, est, o.to(DEV), d.to(DEV), o.shape[0], 1024, render_bkgd=bk, probabilistic=prob, **H.RENDER_KW)
    assert ref["total_samples"] > 4000
    err = {k: float((out[k].cpu() - ref[k]).abs().max()) for k in ("rgb", "acc", "depth", "sem")}
    print(f"render {sc['neurons']}x{sc['layers']} {kw} prob={prob}: max abs " + ", ".join(f"{k} {v:.2e}" for k, v in err.items()))
    check(out, ref, prob)
    other = RD.render_views(H.hip_field(sc, **_flip(kw, flip_key)), est, o.to(DEV), d.to(DEV), o.shape[0], 1024, render_bkgd=bk, probabilistic=prob,
                            **H.RENDER_KW)
    assert not torch.equal(other["sem"], out["sem"]), f"switch has no effect on the render: {flip_key}"


@pytest.mark.parametrize("prob", [False, True])
def test_bf16_render_config2_model(prob):
    """The bf16 unit's fused renderer at BASELINE config 2's model (64 x 4, 29 classes, 256 x 256 view geometry)."""
    sc = H.make_scene("102344250", neurons=64, layers=4, C=29, seed=5)
    kw, okw = _mode(bf16=True)
    _render_case(sc, 2, 20, 256, torch.tensor([0.2, 0.7, 0.4]), kw, okw, "mfma_bf16", prob, _check_render_bf16)


@pytest.mark.parametrize("prob", [False, True])
@pytest.mark.parametrize("bf16", [False, True])
def test_blend_fp16_render(bf16, prob):
    """The configuration of the `render_blend_fp16` bench leg (128 x 2, fp16 blend) in both units, against the oracle's fp16 blend; the fp16 unit
    at test_render_test_matches_oracle's bars."""
    sc = H.make_scene()
    kw, okw = _mode(bf16=bf16, blend=True)
    check = _check_render_bf16 if bf16 else _check_render
    _render_case(sc, 1, 32, 640, torch.tensor([0.1, 0.3, 0.6]), kw, okw, "tcnn_blend_fp16", prob, check)


@pytest.mark.parametrize("prob", [False, True])
def test_bf16_output_fp16_render(prob):
    """bf16 operands with the fp16 hand-over, through the fused renderer (128 x 2)."""
    sc = H.make_scene(log2_hashmap_size=15, head_gain=2.0)
    kw, okw = _mode(bf16=True, out16=True)
    _render_case(sc, 1, 24, 640, torch.zeros(3), kw, okw, "tcnn_output_rounding", prob, _check_render_bf16)


# ------------------------------------------------------------------ f. density pre-pass and presampled steps
@pytest.mark.parametrize("mode", ["bf16", "blend_fp16"])
def test_ray_major_density_prepass_in_other_modes(mode):
    """test_ray_major_density_prepass_gives_same_samples with the bf16 unit's and the B16 `MODE 3` density pass (mnf_field_density_rays): the same
    sample set as every-sample density + visibility, and the pass's densities are the plain density kernel's where it evaluated."""
    from apnrf_amd.ngp import RaySigmaFn
    kw = _mode(bf16=(mode == "bf16"), blend=(mode == "blend_fp16"))[0]
    flip_key = "mfma_bf16" if mode == "bf16" else "tcnn_blend_fp16"
    sc = H.make_scene(log2_hashmap_size=15, seed=3)
    sc["params"] = H.S.make_field_params(seed=3, log2_hashmap_size=15, density_gain=24.0)      # opaque quickly: long invisible tails
    hip, est = H.hip_field(sc, **kw), H.hip_estimator(sc)
    o, d = H.view_rays(sc, 2, h=40, w=40)
    o, d = o.to(DEV), d.to(DEV)
    fast = RaySigmaFn(hip, o, d)
    plain = lambda ts, te, ri: hip.forward_samples(o, d, ri, ts, te, density_only=True)[0]
    for eps, thre in ((1e-4, 0.01), (1e-2, 0.0), (1e-4, 0.0)):
        a = est.sampling(o, d, sigma_fn=fast, near_plane=0.1, render_step_size=1e-3, cone_angle=0.004, alpha_thre=thre, early_stop_eps=eps)
        b = est.sampling(o, d, sigma_fn=plain, near_plane=0.1, render_step_size=1e-3, cone_angle=0.004, alpha_thre=thre, early_stop_eps=eps)
        for x, y in zip(a, b):
            np.testing.assert_array_equal(x.cpu().numpy(), y.cpu().numpy())
        assert a[0].shape[0] > 1000
    n = o.shape[0]
    near, far = torch.full((n,), 0.1, device=DEV), torch.full((n,), 1e10, device=DEV)
    ri, ts, te, info = est._sample_single_pass(o, d, near, far, 1e-3, 0.004)
    s_fast, s_all = fast.ray_major(ts, te, ri, info, 1e-4), plain(ts, te, ri)
    skipped = (s_fast == 0) & (s_all > 0)
    assert 0.03 < float(skipped.float().mean()) < 0.99
    np.testing.assert_array_equal(s_fast[~skipped].cpu().numpy(), s_all[~skipped].cpu().numpy())
    np.testing.assert_array_equal(fast.ray_major(ts, te, ri, info, 0.0).cpu().numpy(), s_all.cpu().numpy())
    # the mode is on in both passes
    other = H.hip_field(sc, **_flip(kw, flip_key))
    assert not torch.equal(RaySigmaFn(other, o, d).ray_major(ts, te, ri, info, 0.0), s_all)
    assert not torch.equal(other.forward_samples(o, d, ri, ts, te, density_only=True)[0], s_all)


def test_bf16_presampled_steps_are_bitwise_the_steps_that_march_themselves():
    """The bitwise core of test_presampled_steps_are_bitwise_the_steps_that_march_themselves in the bf16 unit: steps 15 .. 18 with the occupancy refresh
    at step 16 (whose density pass runs in bf16), presampled or marching themselves, synchronous: same sample counts, same parameters bit for bit."""
    from apnrf_amd import render as RD
    from apnrf_amd.optim import FusedAdam
    sc = H.make_scene(log2_hashmap_size=15)
    bk = torch.tensor([0.3, 0.6, 0.1], device=DEV)
    steps, first = 4, 15
    data = []
    for k in range(steps + 1):
        o, d = H.view_rays(sc, 1 + k % 3, h=36 + 2 * (k % 4), w=40)
        rng = np.random.default_rng(70 + k)
        n = o.shape[0]
        data.append((RD.Rays(o.to(DEV), d.to(DEV)), torch.from_numpy(rng.random((n, 3)).astype(np.float32)).to(DEV),
                     torch.from_numpy(rng.uniform(0.5, 4.0, n).astype(np.float32)).to(DEV), torch.from_numpy(rng.integers(0, sc["C"], n)).to(DEV), bk))
    kw = dict(H.RENDER_KW)

    def run(pre, bf16=True):
        f, e = H.hip_field(sc, mfma_bf16=bf16).train(), H.hip_estimator(sc)
        opt = FusedAdam(f.parameters(), lr=1e-3, eps=1e-15).bind_field(f)
        RD.reserve_sample_bounds(f, 1 << 21, 1 << 20)
        hist, tok, used = [], None, 0
        if pre:
            tok = RD.presample(f, e, data[0][0], seed=900 + first, **kw)
        for k in range(steps):
            step = first + k                                                      # step 16 refreshes the occupancy grid: the tokens for 16 and 17 are stale
            nxt = RD.presample(f, e, data[k + 1][0], seed=900 + step + 1, **kw) if pre else None
            torch.manual_seed(1000 + step)
            out = RD.train_step(f, e, opt, *data[k], step=step, sync=True, deterministic=True, presampled=tok, seed=900 + step, **kw)
            used += int(tok is not None and tok.adopted)
            hist.append(int(out["n_rendering_samples"]))
            tok = nxt
        torch.cuda.synchronize()
        return hist, [p.detach().clone() for p in f.parameters() if p.numel()], used

    n_a, p_a, _ = run(False)
    n_b, p_b, used = run(True)
    assert used == steps - 2 and n_a == n_b and min(n_a) > 3000, (used, n_a, n_b)
    for a, b in zip(p_a, p_b):
        assert torch.equal(a, b)
    _, p_c, _ = run(False, bf16=False)
    assert not all(torch.equal(a, c) for a, c in zip(p_a, p_c))                   # the bf16 unit really ran
