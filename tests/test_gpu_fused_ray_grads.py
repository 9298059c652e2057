"""GPU tests of the fused train render's ray gradients: `render.fused_train_render_rays` (`mnf_train_render_backward_rays`: the step's
backward, then `train_render_ray_grad_kernel` of csrc/inputgrad.hip), with trainable and with frozen parameters.

Reference: torch autograd through the oracle — `oracle.render.sem_rendering` on the sample set `oracle.render.render_train` returns in its extras, with the
rays requiring a gradient (the sample set is a constant of the render, as on the drop-in route).  Bars: the project's own for this backward
(test_gpu_train_render.py's gradient groups): rel L2 < 3e-2 and cosine > 0.999, in bf16 6e-2 / 0.998 — the ray gradients are linear in the dX and dZr1 those
groups are made of.  Every figure is printed before it is asserted; the figures against the drop-in route are printed without a bar.

Batch: test_gpu_train_render.py's `_case` (13 x 14 view of pose 4 + 11 rays that miss the box = 193 rays, background (0.5, 0.2, 0.9), no jitter) for the
shapes (128, 2, 29) and (64, 4, 13); its oracle render is computed once and shared with that file's tests."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import helpers as H
from apnrf_amd import _lib as L
from test_gpu_input_grads import _figures
from test_gpu_train_render import BK, N_MISS, _case, _check_grads, _check_planes, _loss, _params

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(128, 2, 29), (64, 4, 13)]
F16_BAR = dict(rel=3e-2, cos=0.999)
BF16_BAR = dict(rel=6e-2, cos=0.998)
INVALID, WORKSPACE = -1, -4


def _close(got, want, name, rel, cos):
    err, c = _figures(got, want)
    print(f"{name}: rel L2 err {err:.3e}, cos {c:.6f}  (bar {rel:g}, {cos:g})")
    assert err < rel and c > cos, f"{name}: rel L2 err {err:.3e}, cos {c:.6f}"


def _loss4(rgb, acc, depth, sem, pix, dep, lab):
    """all four planes: the reference's three-term loss plus a term on the opacity"""
    return _loss(rgb, depth, sem, pix, dep, lab) + 0.1 * (acc - 1.0).abs().mean()


def _mode_case(mode):
    """`_case` for a precision mode: (case, field_kw, bar).  bf16 is one of `_case`'s own; the two tcnn modes get an oracle in that mode and its own render."""
    if mode == "mfma_bf16":
        c = _case(128, 2, 29, True)
        return c, c["field_kw"], BF16_BAR
    return _tcnn_case(mode), {mode: True}, F16_BAR


@functools.lru_cache(maxsize=None)
def _tcnn_case(mode):
    from oracle import render as R
    from test_gpu_train_render import _targets, _with_misses
    sc = H.make_scene(neurons=128, layers=2, C=29, log2_hashmap_size=15)      # (the fp16 blend is built for 128 neurons only)
    o, d = _with_misses(sc, *H.view_rays(sc, 4, h=13, w=14))
    n = o.shape[0]
    okw = dict(blend="f16") if mode == "tcnn_blend_fp16" else dict(output_rounding=True)
    orc = H.oracle_field(sc, requires_grad=True, **okw)
    est = H.hip_estimator(sc)
    ref = R.render_train(orc, sc["occ"], est.aabbs.cpu().numpy(), float(est.occs.mean().item()), o, d, torch.full((n,), 0.1), render_bkgd=BK,
                         render_step_size=1e-3, cone_angle=0.004, alpha_thre=0.01)
    pix, dep, lab = _targets(n, 29)
    return dict(sc=sc, o=o, d=d, n=n, orc=orc, est=est, ref=ref, pix=pix, dep=dep, lab=lab, field_kw={mode: True})


_ORACLE = {}


def _oracle(c):
    """The oracle's loss and its gradients with respect to the rays and the parameters on the case's own sample set, computed once per case
    (`torch.autograd.grad`: nothing of the shared case is written).  Asserts what the batch is chosen for."""
    key = id(c)
    if key not in _ORACLE:
        from oracle import render as R
        ex = c["ref"][5]
        ri, ts, te = ex["ray_indices"], ex["t_starts"], ex["t_ends"]
        per_ray = torch.bincount(ri, minlength=c["n"])
        print(f"oracle sample set: {ts.shape[0]} kept samples, per-ray counts {int(per_ray[per_ray > 0].min())} .. {int(per_ray.max())}, "
              f"{int((per_ray > 63).sum())} rays above 63, {int((per_ray > 128).sum())} above 128, {int((per_ray == 0).sum())} rays keep none")
        assert int(per_ray.max()) > 64, "the longest ray must cross a 64-sample tile"
        assert ts.shape[0] % 64 != 0, "the total must not be a multiple of the tile"
        assert int((per_ray == 0).sum()) >= 1 and bool((per_ray[-N_MISS:] == 0).all()), "at least one ray keeps nothing"
        o, d = c["o"].clone().requires_grad_(), c["d"].clone().requires_grad_()
        orc = c["orc"]
        planes = R.sem_rendering(orc, o, d, ts, te, ri, c["n"], BK)[:4]
        loss = _loss4(*planes, c["pix"], c["dep"], c["lab"])
        g = torch.autograd.grad(loss, [o, d, orc.p_base, orc.p_head, orc.p_sem])
        _ORACLE[key] = dict(loss=loss.detach(), g_o=g[0], g_d=g[1], g_params=g[2:], n=ts.shape[0])
    return _ORACLE[key]


def _run(c, field_kw=None, freeze=False, req_o=True, req_d=True, deterministic=False, ray_gradients=True, loss_factor=None, rays=None, fused=True):
    """One render + backward of the case's batch on a fresh field -> dict(hip, o, d, planes, n, loss)"""
    from apnrf_amd import render as RD
    hip = H.hip_field(c["sc"], **(c["field_kw"] if field_kw is None else field_kw)).train()
    if freeze:
        for prm in hip.parameters():
            prm.requires_grad_(False)
    if rays is None:
        o, d = c["o"].to(DEV).requires_grad_(req_o), c["d"].to(DEV).requires_grad_(req_d)
        rays = RD.Rays(o, d)
    pix, dep, lab = (t.to(DEV) for t in (c["pix"], c["dep"], c["lab"]))
    kw = dict(render_bkgd=BK.to(DEV), **H.RENDER_KW)
    if fused:
        render = RD.fused_train_render_rays if ray_gradients else RD.fused_train_render
        out = render(hip, c["est"], rays, stratified=False, deterministic=deterministic, **kw)
    else:
        hip.eval()      # (the drop-in's jitter follows the mode)
        out = RD.render_image_with_occgrid_with_depth_guide(hip, c["est"], rays, **kw)
    flat = [x.reshape(-1, x.shape[-1]) for x in out[:4]]
    n_rays = flat[0].shape[0]
    loss = _loss4(*flat, pix[:n_rays], dep[:n_rays], lab[:n_rays])
    if loss_factor is not None:
        loss = loss * loss_factor
    loss.backward()
    return dict(hip=hip, o=rays.origins, d=rays.viewdirs, planes=flat, n=out[4], loss=loss.detach())


_FIRST = {}


def _first(shape):
    """Case 1's run of a shape (trainable parameters, both rays requiring a gradient), made once: the bits cases 2, 3, 7 and 8 are compared with"""
    if shape not in _FIRST:
        c = _case(*shape)
        r = _run(c)
        _FIRST[shape] = dict(g_o=r["o"].grad.clone(), g_d=r["d"].grad.clone(), run=r)
    return _FIRST[shape]


def _launches(fn, labels):
    lib = L.load_library()
    lib.mnf_profile_begin()
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        lib.mnf_profile_end(None, None)
    out = {}
    for label in labels:
        cnt = ctypes.c_int64()
        lib.mnf_profile_query(label.encode(), None, ctypes.byref(cnt))
        out[label] = cnt.value
    return out


# ------------------------------------------------------------------ 1. values
@pytest.mark.parametrize("shape", SHAPES)
def test_values_match_oracle(shape):
    """Planes, sample count, g_o, g_d and the parameter gradients of one render + backward against the oracle; the rays that miss the box get exact zeros.
    (The parent commit has no `fused_train_render_rays`.)"""
    from apnrf_amd import render as RD
    c = _case(*shape)
    want = _oracle(c)
    first = _first(shape)
    r = first["run"]
    assert RD.latest_train_render(r["hip"]) is not None                      # the fused route, not the hand-over
    assert r["n"] == want["n"] == c["ref"][4]
    _check_planes(r["planes"], c["ref"])
    print(f"loss {float(r['loss']):.6f} vs oracle {float(want['loss']):.6f}; max |g_o| {float(want['g_o'].abs().max()):.3e}, max |g_d| {float(want['g_d'].abs().max()):.3e}")
    np.testing.assert_allclose(float(r["loss"]), float(want["loss"]), rtol=1e-4)
    _close(first["g_o"], want["g_o"], "g_o", **F16_BAR)
    _close(first["g_d"], want["g_d"], "g_d", **F16_BAR)
    _check_grads([p.grad for p in _params(r["hip"])], c["orc"], want["g_params"])
    assert first["g_o"].shape == (c["n"], 3) and first["g_d"].shape == (c["n"], 3)
    assert bool((first["g_o"][-N_MISS:] == 0).all()) and bool((first["g_d"][-N_MISS:] == 0).all())
    assert bool((want["g_o"][-N_MISS:] == 0).all()) and bool((want["g_d"][-N_MISS:] == 0).all())
    drop = _run(c, fused=False)      # the drop-in route with the same rays requiring gradients: figures only
    for name, got, ref in (("g_o", first["g_o"], drop["o"].grad), ("g_d", first["g_d"], drop["d"].grad)):
        err, cs = _figures(got, ref)
        print(f"{name} against the drop-in route: rel L2 {err:.3e}, cos {cs:.6f}  (no bar)")


# ------------------------------------------------------------------ 2. frozen parameters
@pytest.mark.parametrize("shape", SHAPES)
def test_frozen_parameters(shape):
    """No parameter gradient, the ray gradients' bits are case 1's, and the backward launches dgrad and the ray kernel but neither wgrad nor the scatter"""
    c = _case(*shape)
    first = _first(shape)
    box = {}
    counts = _launches(lambda: box.update(_run(c, freeze=True)), ("dgrad", "wgrad", "hash_scatter", "hash_scatter_bins", "train_render_ray_grad"))
    print("launches with frozen parameters:", counts)
    assert all(prm.grad is None for prm in box["hip"].parameters())
    assert torch.equal(box["o"].grad, first["g_o"]) and torch.equal(box["d"].grad, first["g_d"])
    assert counts["dgrad"] >= 1 and counts["wgrad"] == 0 and counts["hash_scatter"] == 0 and counts["hash_scatter_bins"] == 0
    assert counts["train_render_ray_grad"] == 1
    trainable = _launches(lambda: _run(c), ("dgrad", "wgrad", "hash_scatter", "train_render_ray_grad"))
    print("launches with trainable parameters:", trainable)
    assert trainable["wgrad"] >= 1 and trainable["hash_scatter"] >= 1 and trainable["train_render_ray_grad"] == 1


# ------------------------------------------------------------------ 3. only what is asked
def test_only_what_is_asked():
    c = _case(*SHAPES[0])
    first = _first(SHAPES[0])
    r = _run(c, req_d=False)
    assert r["d"].grad is None and torch.equal(r["o"].grad, first["g_o"])
    r = _run(c, req_o=False, freeze=True)
    assert r["o"].grad is None and torch.equal(r["d"].grad, first["g_d"])


# ------------------------------------------------------------------ 4. parameter gradients unchanged
def test_parameter_gradients_unchanged():
    """deterministic=True: the three parameter gradients behind a ray-gradient backward are the bits of a plain `fused_train_render` backward"""
    c = _case(*SHAPES[0])
    with_rays = _run(c, deterministic=True)
    plain = _run(c, deterministic=True, req_o=False, req_d=False, ray_gradients=False)
    assert plain["o"].grad is None and with_rays["o"].grad is not None
    for a, b in zip(_params(with_rays["hip"]), _params(plain["hip"])):
        assert float(a.grad.abs().max()) > 0 and torch.equal(a.grad, b.grad)


# ------------------------------------------------------------------ 5. other precision modes
@pytest.mark.parametrize("mode", ["mfma_bf16", "tcnn_blend_fp16", "tcnn_output_rounding"])
def test_other_precision_modes(mode):
    c, field_kw, bar = _mode_case(mode)
    want = _oracle(c)
    r = _run(c, field_kw=field_kw)
    print(f"{mode}: {r['n']} samples (oracle {want['n']}), loss {float(r['loss']):.6f} vs {float(want['loss']):.6f}")
    assert r["n"] == want["n"]
    _close(r["o"].grad, want["g_o"], f"g_o ({mode})", **bar)
    _close(r["d"].grad, want["g_d"], f"g_d ({mode})", **bar)


# ------------------------------------------------------------------ 6. a non-finite incoming gradient
def test_non_finite_gradient_gives_zeros():
    from apnrf_amd import render as RD
    c = _case(*SHAPES[0])
    r = _run(c, deterministic=True, loss_factor=float("nan"))
    last = RD.latest_train_render(r["hip"])
    status, skip = int(last["counts"][3]), int(last["skip"])
    print(f"status {status}, skip {skip}")
    assert status & 32 and skip > 0
    assert r["o"].grad.shape == (c["n"], 3) and bool((r["o"].grad == 0).all()) and bool((r["d"].grad == 0).all())
    assert all(bool((prm.grad == 0).all()) for prm in _params(r["hip"]))


# ------------------------------------------------------------------ 7. shapes
def test_ray_shapes_and_second_backward():
    from apnrf_amd import render as RD
    c = _case(*SHAPES[0])
    first = _first(SHAPES[0])
    o, d = c["o"].to(DEV), c["d"].to(DEV)
    # [2, 91, 3] views of the first 182 rays: a batch of its own (the miss rays are left out), so compare with a flat render of the same 182 rays
    flat = _run(c, rays=RD.Rays(o[:182].clone().requires_grad_(), d[:182].clone().requires_grad_()))
    img = _run(c, rays=RD.Rays(o[:182].view(2, 91, 3).clone().requires_grad_(), d[:182].view(2, 91, 3).clone().requires_grad_()))
    assert img["o"].grad.shape == (2, 91, 3) and img["d"].grad.shape == (2, 91, 3)
    assert torch.equal(img["o"].grad.view(-1, 3), flat["o"].grad) and torch.equal(img["d"].grad.view(-1, 3), flat["d"].grad)
    # a non-contiguous slice: every second row of a [386, 3] tensor is the batch of case 1
    wide_o, wide_d = torch.zeros(2 * c["n"], 3, device=DEV), torch.zeros(2 * c["n"], 3, device=DEV)
    wide_o[::2], wide_d[::2] = o, d
    wide_o.requires_grad_(); wide_d.requires_grad_()
    so, sd = wide_o[::2], wide_d[::2]
    assert not so.is_contiguous()
    so.retain_grad(); sd.retain_grad()
    r = _run(c, rays=RD.Rays(so, sd))
    assert so.grad.shape == (c["n"], 3) and torch.equal(so.grad, first["g_o"]) and torch.equal(sd.grad, first["g_d"])
    assert torch.equal(wide_o.grad[::2], first["g_o"]) and bool((wide_o.grad[1::2] == 0).all())
    # one backward per render
    hip = H.hip_field(c["sc"]).train()
    ro, rd = o.clone().requires_grad_(), d.clone().requires_grad_()
    planes = RD.fused_train_render_rays(hip, c["est"], RD.Rays(ro, rd), render_bkgd=BK.to(DEV), stratified=False, **H.RENDER_KW)
    loss = planes[0].sum()
    loss.backward(retain_graph=True)
    with pytest.raises(L.MnfError):
        loss.backward()


# ------------------------------------------------------------------ 8. same bits
def test_same_inputs_same_bits():
    c = _case(*SHAPES[1])
    first = _first(SHAPES[1])
    again = _run(c)
    assert torch.equal(again["o"].grad, first["g_o"]) and torch.equal(again["d"].grad, first["g_d"])
    assert float(first["g_o"].abs().max()) > 0 and float(first["g_d"].abs().max()) > 0


# ------------------------------------------------------------------ 9. C ABI argument errors
def test_argument_errors_enqueue_nothing():
    from apnrf_amd import render as RD
    lib = L.load_library()
    c = _case(*SHAPES[0])
    hip = H.hip_field(c["sc"]).train()
    rays = RD.Rays(c["o"].to(DEV), c["d"].to(DEV))
    call = RD._launch_train_render(RD._train_state(hip), hip, c["est"], rays, BK.to(DEV), 0, True, stratified=False, deterministic=False, early_stop_eps=1e-4,
                                   far_plane=1e10, **H.RENDER_KW)
    R_, (cap_m, cap_k) = call["_rays"], call["_caps"]
    g_rgb = torch.ones(R_, 3, device=DEV)
    outs = dict(g_o=torch.full((R_, 3), 7.0, device=DEV), g_d=torch.full((R_, 3), 7.0, device=DEV),
                base=torch.full_like(hip.mlp_base.params, 7.0), head=torch.full_like(hip.mlp_head.params, 7.0), sem=torch.full_like(hip.mlp_sem.params, 7.0))

    def opts_with(**kw):
        o = type(call["_opts"]).from_buffer_copy(call["_opts"])
        for k, v in kw.items():
            setattr(o, k, v)
        return o

    def rc_of(opts=None, dirs=True, g_o=True, g_d=True, params=(True, True, True), n_rays=R_, max_marched=cap_m, max_kept=cap_k, ws=True, nbytes=call["_nbytes"]):
        p = [L.ptr(outs[k]) if w else None for k, w in zip(("base", "head", "sem"), params)]
        rc = lib.mnf_train_render_backward_rays(call["_handle"], n_rays, ctypes.byref(opts if opts is not None else call["_opts"]),
                                                L.ptr(call["_dirs"]) if dirs else None, L.ptr(g_rgb), 3, 1, None, 0, None, 0, None, 0, 0, *p,
                                                L.ptr(outs["g_o"]) if g_o else None, L.ptr(outs["g_d"]) if g_d else None, L.ptr(call["counts"]),
                                                L.ptr(call["skip"]), max_marched, max_kept, L.ptr(call["_ws"]) if ws else None, nbytes, L.stream())
        torch.cuda.synchronize()
        return rc

    cases = [("both ray outputs NULL", dict(g_o=False, g_d=False), INVALID),
             ("one parameter pointer NULL", dict(params=(True, False, True)), INVALID), ("two parameter pointers NULL", dict(params=(False, True, False)), INVALID),
             ("g_rays_d without rays_d", dict(dirs=False), INVALID), ("presampled set", dict(opts=opts_with(presampled=1)), INVALID),
             ("wrong struct_size", dict(opts=opts_with(struct_size=call["_opts"].struct_size - 4)), INVALID),
             ("n_rays 0", dict(n_rays=0), INVALID), ("max_marched 0", dict(max_marched=0), INVALID), ("max_kept -1", dict(max_kept=-1), INVALID),
             ("workspace one byte short", dict(nbytes=call["_nbytes"] - 1), WORKSPACE), ("workspace NULL", dict(ws=False), WORKSPACE)]

    def run():
        for name, kw, want in cases:
            rc = rc_of(**kw)
            assert rc == want, (name, rc, lib.mnf_last_error())
            assert all(bool((t == 7.0).all()) for t in outs.values()), name      # nothing was written
    counts = _launches(run, ("train_render_ray_grad", "dgrad"))
    assert counts == {"train_render_ray_grad": 0, "dgrad": 0}, counts
    # the same arguments without an error: the call goes through, origins alone and frozen
    assert rc_of(dirs=False, g_d=False, params=(False, False, False)) == 0
    assert bool((outs["g_o"] != 7.0).any()) and bool((outs["g_d"] == 7.0).all()) and bool((outs["base"] == 7.0).all())


# ------------------------------------------------------------------ 10. the pose vector, end to end
def test_pose_vector_gradient_matches_oracle():
    """d(L2 photometric loss against the un-perturbed render)/d(rotvec, trans) through `transform_rays` and `fused_train_render_rays` with
    frozen parameters, against the same chain through the oracle: `render_train` on the transformed rays (detached) gives the oracle's sample set,
    `sem_rendering` on it the differentiable render.  Each side's target is its own un-perturbed render.  Bar: rel L2 < 2e-2 on the 6-vector, what
    test_gpu_input_grads.py::test_pose_vector_gradient_matches_oracle holds the drop-in to."""
    from apnrf_amd import render as RD
    from oracle import render as R
    sc = H.make_scene(neurons=64, layers=2, C=5, log2_hashmap_size=12)
    hip, orc, est = H.hip_field(sc).train(), H.oracle_field(sc), H.hip_estimator(sc)
    o, d = H.view_rays(sc, 1, h=8, w=8)
    o, d = o.float().contiguous(), d.float().contiguous()
    n_rays = o.shape[0]
    xi = np.array([0.01, -0.02, 0.015, 0.02, -0.01, 0.015], np.float32)
    for prm in hip.parameters():
        prm.requires_grad_(False)
    kw = dict(stratified=False, **H.RENDER_KW)
    with torch.no_grad():
        target = RD.fused_train_render(hip, est, RD.Rays(o.to(DEV), d.to(DEV)), **kw)[0]
    rot, tr = torch.from_numpy(xi[:3].copy()).to(DEV).requires_grad_(), torch.from_numpy(xi[3:].copy()).to(DEV).requires_grad_()
    rays = RD.transform_rays(RD.Rays(o.to(DEV), d.to(DEV)), rot, tr)
    rgb, _, _, _, n = RD.fused_train_render_rays(hip, est, rays, **kw)
    assert RD.latest_train_render(hip) is not None
    loss = ((rgb - target) ** 2).mean()
    loss.backward()
    assert all(prm.grad is None for prm in hip.parameters())

    def oracle_samples(ro, rd):
        return R.render_train(orc, sc["occ"], est.aabbs.cpu().numpy(), float(est.occs.mean().item()), ro, rd, torch.full((n_rays,), 0.1),
                              render_step_size=1e-3, cone_angle=0.004, alpha_thre=0.01)
    with torch.no_grad():
        r_target = oracle_samples(o, d)[0]
    r_rot, r_tr = torch.from_numpy(xi[:3].copy()).requires_grad_(), torch.from_numpy(xi[3:].copy()).requires_grad_()
    r_rays = RD.transform_rays(RD.Rays(o, d), r_rot, r_tr)                 # pure torch: the same transform on the CPU
    with torch.no_grad():
        ex = oracle_samples(r_rays.origins.detach(), r_rays.viewdirs.detach())[5]
    r_rgb = R.sem_rendering(orc, r_rays.origins, r_rays.viewdirs, ex["t_starts"], ex["t_ends"], ex["ray_indices"], n_rays)[0]
    r_loss = ((r_rgb - r_target) ** 2).mean()
    r_loss.backward()
    got, want = torch.cat([rot.grad, tr.grad]).cpu(), torch.cat([r_rot.grad, r_tr.grad])
    err, cs = _figures(got, want)
    print(f"{n} kept samples (oracle {ex['t_starts'].shape[0]}); loss {loss.item():.4e} (oracle {r_loss.item():.4e}); pose gradient {got.numpy()} vs "
          f"{want.numpy()}: rel L2 {err:.3e}, cos {cs:.6f}")
    assert err < 2e-2, err
