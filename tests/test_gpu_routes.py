"""GPU parity tests for the routes the host code picks from the field's shape and the batch size: the backward of every compiled (neurons, layers)
pair with the semantic head at its padding edges, the hash-gradient scatter for every split of the 16 levels into replica / walk / binned levels,
the fused train step of every shape, the single-pass sampler with more than one ray per wave, the render marcher reading the occupancy bits from
global memory, and every bucket of the device prefix sum.  Each is compared with the oracle (or numpy) at the tolerances of the parity tests."""
import numpy as np
import pytest
import torch

import helpers as H
from test_gpu_parity import _grad_close
from test_gpu_round6 import _check_grads, _loss, _targets

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ------------------------------------------------------------------ field backward (csrc/train.hip dgrad_kernel<W,NH>, wgrad; csrc/scatter.hip)
def _backward_vs_oracle(neurons, layers, C, lh, n, seed, field_kw=None, oracle_kw=None, rel=2e-2, cos=0.9995, fwd_atol=1e-3, flip_kw=None):
    """test_field_backward_matches_oracle's comparison at one shape: train forward == inference forward, every gradient group within 2e-2 relative L2
    and cosine > 0.9995, untouched table entries exactly zero.  Returns (hip, orc, n_mlp) for further checks.
    field_kw / oracle_kw: the field's precision mode (hip_field keywords) and the oracle of the same mode (oracle_field keywords); rel / cos / fwd_atol: that
    mode's bars.  flip_kw: hip_field keywords of the same route with the mode switch flipped, whose gradients must differ (the switch is really on)."""
    sc = H.make_scene(neurons=neurons, layers=layers, C=C, log2_hashmap_size=lh, head_gain=2.0)
    hip = H.hip_field(sc, **(field_kw or {})).train()
    orc = H.oracle_field(sc, requires_grad=True, **(oracle_kw or {}))
    rng = np.random.default_rng(seed)
    a = sc["aabb"]
    pos = (rng.random((n, 3)) * (a[3:] - a[:3]) * 0.98 + a[:3] + 0.01 * (a[3:] - a[:3])).astype(np.float32)
    pos[:5] = a[:3] - 1.0                                          # outside the box: density gradient must vanish
    d = rng.normal(size=(n, 3)).astype(np.float32); d /= np.linalg.norm(d, axis=-1, keepdims=True)
    g_rgb = (rng.normal(size=(n, 3)) * 1e-3).astype(np.float32)
    g_sig = (rng.normal(size=(n, 1)) * 1e-5).astype(np.float32)
    g_sem = (rng.normal(size=(n, C)) * 1e-3).astype(np.float32)
    rgb, sigma, sem = hip(_cu(pos), _cu(d))
    assert rgb.requires_grad and sem.requires_grad and sem.shape == (n, C)
    torch.autograd.backward([rgb, sigma, sem], [_cu(g_rgb), _cu(g_sig), _cu(g_sem)])
    r_rgb, r_sigma, r_sem = orc(torch.from_numpy(pos), torch.from_numpy(d))
    np.testing.assert_allclose(rgb.detach().cpu().numpy()[5:], r_rgb.detach().numpy()[5:], atol=fwd_atol)  # train forward == inference forward
    torch.autograd.backward([r_rgb, r_sigma, r_sem], [torch.from_numpy(g_rgb), torch.from_numpy(g_sig), torch.from_numpy(g_sem)])
    n_mlp = sum(o * i for o, i in orc.shapes["base"])
    _grad_close(hip.mlp_base.params.grad[:n_mlp], orc.p_base.grad[:n_mlp], "base mlp", rel=rel, cos=cos)
    _grad_close(hip.mlp_base.params.grad[n_mlp:], orc.p_base.grad[n_mlp:], "hash table", rel=rel, cos=cos)
    _grad_close(hip.mlp_head.params.grad, orc.p_head.grad, "rgb head", rel=rel, cos=cos)
    _grad_close(hip.mlp_sem.params.grad, orc.p_sem.grad, "sem head", rel=rel, cos=cos)
    # the semantic output layer class by class (rows of [ceil16(C), neurons / 2]): a wrong row at the padding edge is diluted in the group
    # total; the padding rows get exactly zero
    pad, wh = orc.cfg.sem_out_pad, neurons // 2
    got_w, want_w = hip.mlp_sem.params.grad[-pad * wh:].view(pad, wh), orc.p_sem.grad[-pad * wh:].view(pad, wh)
    for c in range(C):
        _grad_close(got_w[c], want_w[c], f"sem output row {c} of {C}", rel=rel, cos=cos)
    assert bool((got_w[C:] == 0).all()) and bool((want_w[C:] == 0).all())
    untouched = (orc.p_base.grad[n_mlp:] == 0).numpy()
    assert (hip.mlp_base.params.grad[n_mlp:].cpu().numpy()[untouched] == 0).all()
    if flip_kw is not None:
        other = H.hip_field(sc, **flip_kw).train()
        torch.autograd.backward(list(other(_cu(pos), _cu(d))), [_cu(g_rgb), _cu(g_sig), _cu(g_sem)])
        for a, b in zip(hip.parameters(), other.parameters()):
            if a.numel():
                assert not torch.equal(a.grad, b.grad), "the mode switch does not change the backward"
    return hip, orc, n_mlp


@pytest.mark.parametrize("neurons,layers,C,lh", [(128, 1, 1, 12), (128, 2, 16, 15), (128, 3, 17, 19), (128, 4, 32, 12),
                                                 (64, 1, 17, 15), (64, 2, 32, 19), (64, 3, 16, 12), (64, 4, 1, 19)])
def test_field_backward_every_shape(neurons, layers, C, lh):
    """Every (neurons, layers) instantiation of the backward, each with a semantic class count at a padding edge of the head (rows padded to
    ceil16(C): C = 1, 16, 17, 32) and a table size of 2^12 / 2^15 / 2^19; ragged n, a few positions outside the box."""
    _backward_vs_oracle(neurons, layers, C, lh, n=3000 + 21, seed=7)


@pytest.mark.parametrize("lh,n", [(8, 9000), (11, 12000), (12, 8191), (12, 8192), (21, 12000), (22, 12000)])
def test_field_backward_scatter_routes(lh, n):
    """The table gradient's scatter splits the 16 levels by table size and batch size: leading dense levels into private replicas (up to 131 072
    entries), the rest of the walk, and the binned pass (n >= 8192, hashed levels of one power-of-two size up to 2^21 entries).  2^8 / 2^11: every
    level hashed, no replicas, no bins; 2^12: one bin per level, on either side of n = 8192; 2^21: 512 bins (the limit); 2^22: over the limit, walk
    only.  Checked per parameter group and level by level, so that a route that drops or double-counts one level fails on its own."""
    hip, orc, n_mlp = _backward_vs_oracle(128, 2, 29, lh, n=n, seed=17 + lh)
    _, _, size, off, hashed = hip.grid_meta()
    assert sum(size) * 4 == orc.p_base.grad.numel() - n_mlp
    got = hip.mlp_base.params.grad[n_mlp:].view(-1, 4)
    want = orc.p_base.grad[n_mlp:].view(-1, 4)
    for lvl in range(16):
        sl = slice(off[lvl], off[lvl] + size[lvl])
        _grad_close(got[sl], want[sl], f"table level {lvl} ({size[lvl]} entries, hashed={hashed[lvl]})")


# ------------------------------------------------------------------ fused train step (mnf_train_step) of every shape
def _fused_step_vs_oracle(neurons, layers, C, lh, hw, min_samples, field_kw=None, oracle_kw=None, loss_rtol=1e-4, rel=3e-2, cos=0.999, flip_kw=None,
                          options=None, scene_seed=0, pose=4, image=256):
    """test_config2_fused_train_step_64x4_matches_oracle_autograd's comparison at one shape: one `train_step(fused=True)` against the oracle's
    autograd on the same batch — sample count equal, loss to 1e-4 relative, every gradient group within the train-step tolerance.
    field_kw / oracle_kw: the field's precision mode and the oracle of the same mode; loss_rtol / rel / cos: that mode's bars; flip_kw: hip_field keywords of
    the same step with the mode switch flipped, whose gradients must differ (the switch is really on).
    options: None — the yaml's four (`H.RENDER_KW`) through `train_step`; a dict of render options (`far_plane` and `early_stop_eps` among them, which
    `train_step` pins) — the same comparison through `fused_forward_backward`, with `est.occs` a constant 0.05 (so `occs.mean()` is 0.05), the marched count
    compared too, and the oracle's render, the batch and both fields handed back in the result for further checks.  scene_seed / pose / image: the
    parameters' seed, the view and its full size."""
    from apnrf_amd import render as RD
    from apnrf_amd.optim import FusedAdam
    from oracle import render as R
    sc = H.make_scene("102344250", neurons=neurons, layers=layers, C=C, log2_hashmap_size=lh, seed=scene_seed)
    hip, orc, est = H.hip_field(sc, **(field_kw or {})), H.oracle_field(sc, requires_grad=True, **(oracle_kw or {})), H.hip_estimator(sc)
    o, d = H.view_rays(sc, pose, width=image, height=image, h=hw, w=hw)
    n = o.shape[0]
    pix, dep, lab = _targets(n, C)
    bk = torch.tensor([0.5, 0.2, 0.9])
    rays = RD.Rays(o.to(DEV), d.to(DEV))
    if options is None:
        opt = FusedAdam(hip.parameters(), lr=1e-3, eps=1e-15).bind_field(hip)
        out = RD.train_step(hip, est, opt, rays, pix.to(DEV), dep.to(DEV), lab.to(DEV), bk.to(DEV), step=1, fused=True, sync=True, stratified=False, **H.RENDER_KW)
        assert not out["skipped"]
        kw = dict(H.RENDER_KW)
    else:
        est.occs = torch.full_like(est.occs, 0.05)
        out = RD.fused_forward_backward(hip.train(), est, rays, pix.to(DEV), dep.to(DEV), lab.to(DEV), bk.to(DEV), stratified=False, **options)
        assert out is not None, "the fused route handed over"
        assert int(out["skip"]) == 0 and int(out["counts"][3]) == 0, out["counts"].tolist()
        kw = dict(options)
    assert out["n_rendering_samples"] >= min_samples, out["n_rendering_samples"]
    ref = R.render_train(orc, sc["occ"], est.aabbs.cpu().numpy(), float(est.occs.mean().item()), o, d, torch.full((n,), kw.pop("near_plane")), render_bkgd=bk, **kw)
    r_loss = _loss(ref[0], ref[2], ref[3], pix, dep, lab)
    r_loss.backward()
    if options is not None:
        print(f"fused step {neurons}x{layers} C={C} {field_kw or ''} {options}: kept {out['n_rendering_samples']} vs oracle {ref[4]}, marched {out['n_marched']} vs "
              f"{ref[5]['n_all']}, longest ray {int(out['counts'][2])}, loss rel err {abs(float(out['loss']) / float(r_loss.detach()) - 1.0):.2e}")
        assert out["n_marched"] == int(out["counts"][0]) == ref[5]["n_all"], (out["n_marched"], ref[5]["n_all"])
        out.update(ref=ref, ref_loss=r_loss.detach(), orc=orc, hip=hip, est=est, sc=sc, rays=rays, targets=(pix, dep, lab), bk=bk)
    if field_kw:
        print(f"fused step {neurons}x{layers} C={C} T=2^{lh} {field_kw}: samples {out['n_rendering_samples']} vs oracle {ref[4]}, "
              f"loss rel err {abs(float(out['loss']) / float(r_loss.detach()) - 1.0):.2e}")
    assert ref[4] == out["n_rendering_samples"]
    np.testing.assert_allclose(float(out["loss"]), float(r_loss.detach()), rtol=loss_rtol)
    if C > 1:
        _check_grads(hip, orc, rel=rel, cos=cos)
    else:
        # one class: the cross-entropy is identically zero, so is the semantic head's gradient (oracle: exactly) — the other groups as usual
        assert float(orc.p_sem.grad.abs().max()) == 0.0
        assert float(hip.mlp_sem.params.grad.abs().max()) <= 1e-6 * float(hip.mlp_head.params.grad.abs().max())
        n_mlp = sum(o_ * i_ for o_, i_ in orc.shapes["base"])
        _grad_close(hip.mlp_base.params.grad[:n_mlp], orc.p_base.grad[:n_mlp], "base mlp", rel=rel, cos=cos)
        _grad_close(hip.mlp_base.params.grad[n_mlp:], orc.p_base.grad[n_mlp:], "hash table", rel=rel, cos=cos)
        _grad_close(hip.mlp_head.params.grad, orc.p_head.grad, "rgb head", rel=rel, cos=cos)
    if flip_kw is not None:
        other = H.hip_field(sc, **flip_kw)
        opt2 = FusedAdam(other.parameters(), lr=1e-3, eps=1e-15).bind_field(other)
        out2 = RD.train_step(other, H.hip_estimator(sc), opt2, rays, pix.to(DEV), dep.to(DEV), lab.to(DEV), bk.to(DEV), step=1, fused=True, sync=True,
                             stratified=False, **H.RENDER_KW)
        assert not out2["skipped"]
        assert not torch.equal(hip.mlp_base.params.grad, other.mlp_base.params.grad), "the mode switch does not change the fused step"
    return out


@pytest.mark.parametrize("neurons,layers,C", [(128, 1, 1), (128, 3, 17), (128, 4, 32), (64, 1, 16), (64, 2, 32), (64, 3, 1)])
def test_fused_train_step_every_shape(neurons, layers, C):
    """The six (neurons, layers) pairs the fused step had not been compared at (128 x 2 and 64 x 4 are in test_gpu_parity / test_gpu_round6),
    each with a semantic class count at a padding edge of the head."""
    _fused_step_vs_oracle(neurons, layers, C, 15, hw=20, min_samples=2000)


def test_fused_train_step_config2_exact_shape_binned():
    """BASELINE config 2's exact model — 64 x 4, 29 classes, T = 2^19 — with a batch of >= 8192 samples, so that the fine levels of the table
    gradient go through the binned scatter inside the fused step."""
    _fused_step_vs_oracle(64, 4, 29, 19, hw=24, min_samples=8192)


# ------------------------------------------------------------------ single-pass sampler with several rays per wave (csrc/march.hip sample_rays_kernel)
def _jittered_rays(sc, n, seed=11):
    """n rays from the scene's eight poses (distinct pixels per pose), origins and directions jittered so that no two rays are equal."""
    from oracle import render as R
    rng = np.random.default_rng(seed)
    per = -(-n // 8)
    os_, ds = [], []
    for p in range(8):
        idx = np.sort(rng.choice(640 * 640, per, replace=False))
        o, d = R.generate_image_rays(R.pose_to_c2w(sc["poses"][p]), 640, 640, 320.0, idx)
        os_.append(o.numpy()); ds.append(d.numpy())
    o, d = np.concatenate(os_)[:n], np.concatenate(ds)[:n]
    o = (o + rng.uniform(-1e-2, 1e-2, o.shape)).astype(np.float32)
    d = d + rng.normal(0.0, 1e-3, d.shape)
    d = (d / np.linalg.norm(d, axis=-1, keepdims=True)).astype(np.float32)
    return o, d


@pytest.mark.parametrize("n_rays,stratified", [(8192, False), (8193, True), (16384, False), (16385, False), (40000, True), (262145, False)])
def test_sampler_rays_per_wave_bit_exact(n_rays, stratified):
    """The sampler marches one ray per wave up to 8192 rays, then 2, 4, ... 64 rays per wave (8193 / 16384 -> 2, 16385 -> 4, 40000 -> 8,
    262145 -> 64): lanes > 0 of a wave march rays of their own.  Same samples as the two-pass `traverse_grids` and the oracle marcher, bit for bit."""
    from apnrf_amd import nerfacc as NA
    from oracle import marcher as M
    sc = H.make_scene(log2_hashmap_size=12)
    est = H.hip_estimator(sc)
    o_np, d_np = _jittered_rays(sc, n_rays)
    assert np.unique(np.concatenate([o_np, d_np], 1), axis=0).shape[0] == n_rays
    o, d = _cu(o_np), _cu(d_np)
    step, cone = 1e-3, 0.004
    near = torch.full((n_rays,), 0.1, device=DEV)
    if stratified:
        near = near + torch.rand(n_rays, generator=torch.Generator().manual_seed(5)).to(DEV) * step
    far = torch.full_like(near, 1e10)
    got = est._sample_single_pass(o, d, near, far, step, cone)
    assert got is not None
    ri, ts, te, packed = got
    iv, sm, _ = NA.traverse_grids(o, d, est.binaries, est.aabbs, near_planes=near, far_planes=far, step_size=step, cone_angle=cone)
    np.testing.assert_array_equal(ts.cpu().numpy(), iv.vals[iv.is_left].cpu().numpy())
    np.testing.assert_array_equal(te.cpu().numpy(), iv.vals[iv.is_right].cpu().numpy())
    np.testing.assert_array_equal(ri.cpu().numpy(), sm.ray_indices.cpu().numpy())
    np.testing.assert_array_equal(packed.cpu().numpy(), sm.packed_info.cpu().numpy())
    assert ts.shape[0] > 20 * n_rays
    # the oracle marches the estimator's own box: `aabbs[0]` is the scene box re-derived from centre and extent (occ_grid.py), which can
    # differ from it in the last bits (here -0.2 -> -0.20000005) and move a ray's steps
    ref = M.traverse_grids(o_np, d_np, sc["occ"], est.aabbs.cpu().numpy(), near_planes=near.cpu().numpy(), far_planes=far.cpu().numpy(), step_size=step, cone_angle=cone)
    np.testing.assert_array_equal(ts.cpu().numpy(), ref[0].vals[ref[0].is_left])
    np.testing.assert_array_equal(te.cpu().numpy(), ref[0].vals[ref[0].is_right])
    np.testing.assert_array_equal(ri.cpu().numpy(), ref[1].ray_indices)


# ------------------------------------------------------------------ render marcher with the occupancy bits in global memory (csrc/render.hip)
def _global_grid_case(kind):
    """(field scene, estimator, binaries, rays) of a grid whose bits do not fit the marcher's 64 KB of LDS (levels x cells > 524 288)."""
    from apnrf_amd.nerfacc import OccGridEstimator
    sc = H.make_scene(log2_hashmap_size=15)
    rng = np.random.default_rng(23)
    if kind == "128cube":                                          # nerfacc's default resolution: 2 097 152 cells, one level
        levels, res = 1, [128, 128, 128]
        occ = rng.random((1, 128, 128, 128)) < 0.03
    else:                                                          # the 102344250 grid at four levels: 4 x 163 268 cells
        levels, res = 4, [int(x) for x in sc["res"]]
        occ = np.concatenate([sc["occ"], rng.random((3, *res)) < np.array([0.08, 0.05, 0.04])[:, None, None, None]])
    assert levels * -(-res[0] * res[1] * res[2] // 32) > 16384
    est = OccGridEstimator(torch.from_numpy(sc["aabb"]), resolution=res, levels=levels)
    est.binaries = torch.from_numpy(occ)
    est = est.to(DEV).eval()
    fs = dict(sc); fs["aabb"] = est.aabbs[-1].cpu().numpy().astype(np.float32)      # the field covers the largest level
    o, d = H.view_rays(sc, 3, h=24, w=24)
    return fs, est, occ, o, d


@pytest.mark.parametrize("kind", ["128cube", "102344250x4"])
@pytest.mark.parametrize("prob", [False, True])
def test_render_occupancy_grid_in_global_memory(kind, prob):
    """round_march_kernel<false, false> (one level) and <false, true> (several levels) against the oracle render: sample totals and outputs with the
    bounds of test_multi_level_occupancy_render_matches_oracle."""
    from apnrf_amd import render as RD
    from oracle import render as R
    fs, est, occ, o, d = _global_grid_case(kind)
    hip, orc = H.hip_field(fs), H.oracle_field(fs)
    bk = torch.tensor([0.2, 0.1, 0.4])
    fn = R.render_prob_test if prob else R.render_test
    ref = fn(1024, orc, occ, est.aabbs.cpu().numpy(), o, d, render_bkgd=bk, **H.RENDER_KW)
    out = RD.render_views(hip, est, o.to(DEV), d.to(DEV), o.shape[0], 1024, render_bkgd=bk, probabilistic=prob, **H.RENDER_KW)
    assert ref["total_samples"] > 5000 and len(ref["rounds"]) > 3
    assert abs(int(out["total"][0]) - ref["total_samples"]) <= max(3, 2e-3 * ref["total_samples"]), (int(out["total"][0]), ref["total_samples"])
    for k in ("rgb", "acc", "depth", "sem") + (("rgb_var", "depth_var") if prob else ()):
        assert bool(torch.isfinite(out[k]).all()) and bool(torch.isfinite(ref[k]).all()), k
        err = (out[k].cpu() - ref[k]).abs().reshape(o.shape[0], -1).max(dim=1).values
        assert int((err > 1e-3).sum()) <= 2 and float(err.max()) < 5e-2, (k, float(err.max()), int((err > 1e-3).sum()))


# ------------------------------------------------------------------ device prefix sum (csrc/march.hip exclusive_scan_i64) at its bucket edges
@pytest.mark.parametrize("n", [1, 2047, 2048, 2049, 4096, 4097, 8192, 8193, 16384, 16385])
def test_exclusive_scan_bucket_edges(n):
    """scan_small_kernel<8 | 16 | 32 | 64> up to 2048 / 4096 / 8192 / 16 384 elements, the three-kernel tiled scan above, and the tiled scan whenever
    the input is the output: exact against numpy's cumsum, with and without the total, and through `pack_info`."""
    from apnrf_amd import _lib as L
    from apnrf_amd import nerfacc as NA
    rng = np.random.default_rng(n)
    x = rng.integers(0, 1000, n)
    x[rng.random(n) < 0.2] = 0
    x[-1] = 999                                                    # the last element counts in the total only
    want = np.cumsum(x) - x
    np.testing.assert_array_equal(NA.exclusive_scan_counts(_cu(x)).cpu().numpy(), want)
    st, tot = NA.exclusive_scan_counts(_cu(x), want_total=True)
    np.testing.assert_array_equal(st.cpu().numpy(), want)
    assert int(tot) == int(x.sum())
    ri = rng.integers(0, n, 3 * n + 5)
    cnts = np.bincount(ri, minlength=n)
    np.testing.assert_array_equal(NA.pack_info(_cu(ri), n).cpu().numpy(), np.stack([np.cumsum(cnts) - cnts, cnts], -1))
    # in place through the C ABI
    lib = L.load_library()
    buf = _cu(x)
    total = torch.full((), -1, dtype=torch.int64, device=DEV)
    nbytes = lib.mnf_scan_workspace_bytes(n)
    ws = torch.empty(max(int(nbytes), 8), dtype=torch.uint8, device=DEV)
    L.launch(lib.mnf_exclusive_scan_i64, L.ptr(buf), n, L.ptr(buf), L.ptr(total), L.ptr(ws), nbytes)
    np.testing.assert_array_equal(buf.cpu().numpy(), want)
    assert int(total) == int(x.sum())


# ------------------------------------------------------------------ field forward: the one dispatch row no other test reaches (csrc/field.hip kernel_for)
@pytest.mark.parametrize("bf16", [False, True])
def test_forward_samples_fp16_blend_route(bf16):
    """`mnf_field_forward_samples` with rgb and logits (mode 1, not density-only) and tcnn's fp16 blend: field_kernel<128, NH, 1, false, 0, FEAT_GATHER, true> of
    both units.  The other fp16-blend rows have their tests in test_gpu_precision_modes.py (forward and density on positions, density on samples and ray-major,
    both train forwards, the renderer).  n = 513: nine tiles, two workgroups.  Against the oracle's fp16 blend on the positions the kernel forms, at this file's
    forward bar (rgb and logits 1e-3 absolute, density 2e-3 relative; 8x in the bf16 unit, as test_gpu_precision_modes.BF16)."""
    n, tol = 513, (8.0 if bf16 else 1.0)
    sc = H.make_scene(neurons=128, layers=2, C=17, log2_hashmap_size=12, head_gain=2.0)
    hip = H.hip_field(sc, mfma_bf16=bf16, tcnn_blend_fp16=True)
    orc = H.oracle_field(sc, precision="bf16" if bf16 else "f16", blend="f16")
    o, d = H.view_rays(sc, 3, h=16, w=16)
    rng = np.random.default_rng(2)
    ri = np.sort(rng.integers(0, 256, n))
    ts = rng.uniform(0.2, 4.0, n).astype(np.float32)
    te = ts + 0.003
    with torch.no_grad():
        rgb, sigma, sem = hip.forward_samples(o.to(DEV), d.to(DEV), _cu(ri), _cu(ts), _cu(te))
        plain = H.hip_field(sc, mfma_bf16=bf16).forward_samples(o.to(DEV), d.to(DEV), _cu(ri), _cu(ts), _cu(te))
    pos = o[ri] + d[ri] * (torch.from_numpy(ts) + torch.from_numpy(te))[:, None] / 2.0
    r_rgb, r_sigma, r_sem = orc(pos, d[ri])
    inside = (r_sigma[:, 0] > 0).numpy()
    assert 50 < inside.sum() and (sigma.cpu().numpy() > 0).tolist() == inside.tolist()
    np.testing.assert_allclose(sigma.cpu().numpy(), r_sigma.numpy()[:, 0], rtol=2e-3 * tol, atol=1e-6)
    np.testing.assert_allclose(rgb.cpu().numpy()[inside], r_rgb.numpy()[inside], atol=1e-3 * tol, rtol=0)
    np.testing.assert_allclose(sem.cpu().numpy()[inside], r_sem.numpy()[inside], atol=1e-3 * tol, rtol=2e-3 * tol)
    assert not torch.equal(plain[2], sem) and not torch.equal(plain[1], sigma), "the blend switch has no effect on this route"
