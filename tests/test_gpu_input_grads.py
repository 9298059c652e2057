"""Gradients of the field with respect to its INPUTS (positions, directions, rays): `mnf_field_backward_inputs` / `mnf_ray_input_gradients`
(csrc/inputgrad.hip) behind `NGPRadianceField.forward`, `forward_samples_grad`, `sem_rendering` and `transform_rays`, against torch autograd through
the oracle (`oracle.field.OracleField`, `oracle.render.sem_rendering`: fp32 gradient of the same 16-bit forward).

Bar: the project's own for the gradients of this backward (test_gpu_parity.py `_grad_close`): relative L2 error < 2e-2 and cosine > 0.9995 per gradient
group; in the bf16 unit the bar test_gpu_precision_modes.py applies to bf16 backward gradients (6e-2, 0.998).  dL/dpos is linear in dX and dL/ddir is
linear in dZr1, the quantities the hash-table and head-weight gradients are already held to at that bar.  Every figure is printed before it is asserted."""
import ctypes

import numpy as np
import pytest
import torch

import helpers as H
from apnrf_amd import _lib as L

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F16_BAR = dict(rel=2e-2, cos=0.9995)
BF16_BAR = dict(rel=6e-2, cos=0.998)


def _cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _figures(got, want):
    got, want = got.detach().double().cpu().numpy().ravel(), want.detach().double().cpu().numpy().ravel()
    denom = np.linalg.norm(want)
    assert denom > 0
    return float(np.linalg.norm(got - want) / denom), float(got @ want / (np.linalg.norm(got) * denom + 1e-300))


def _close(got, want, name, rel=2e-2, cos=0.9995):
    err, c = _figures(got, want)
    print(f"{name}: rel L2 err {err:.3e}, cos {c:.6f}  (bar {rel:g}, {cos:g})")
    assert err < rel and c > cos, f"{name}: rel L2 err {err:.3e}, cos {c:.6f}"


def _samples(sc, n, seed):
    """n samples with 5 positions outside the box, unit directions and cotangents sized as test_field_backward_matches_oracle's (the loss-scaled
    fp16 gradients stay far from saturation)"""
    rng = np.random.default_rng(seed)
    a, C = sc["aabb"], sc["C"]
    pos = (rng.random((n, 3)) * (a[3:] - a[:3]) * 0.98 + a[:3] + 0.01 * (a[3:] - a[:3])).astype(np.float32)
    pos[:5] = a[:3] - 1.0 + rng.random((5, 3)).astype(np.float32) * 0.5
    d = rng.normal(size=(n, 3)).astype(np.float32); d /= np.linalg.norm(d, axis=-1, keepdims=True)
    g = ((rng.normal(size=(n, 3)) * 1e-3).astype(np.float32), (rng.normal(size=(n, 1)) * 1e-5).astype(np.float32),
         (rng.normal(size=(n, C)) * 1e-3).astype(np.float32))
    return pos, d, g


def _oracle_input_grads(orc, pos, d, g):
    """(dL/dpos, dL/ddir) by autograd through the oracle; its parameter gradients, if it was built with requires_grad, land in orc.p_*.grad"""
    p, q = torch.from_numpy(pos).requires_grad_(), torch.from_numpy(d).requires_grad_()
    torch.autograd.backward(list(orc(p, q)), [torch.from_numpy(x) for x in g])
    return p.grad, q.grad


def _hip_input_grads(hip, pos, d, g, pos_grad=True, dir_grad=True):
    p, q = _cu(pos).requires_grad_(pos_grad), _cu(d).requires_grad_(dir_grad)
    outs = hip(p, q)
    torch.autograd.backward(list(outs), [_cu(x) for x in g])
    return p, q, outs


# ------------------------------------------------------------------ 1. values
@pytest.mark.parametrize("neurons,layers,C,lh", [(128, 2, 29, 14), (64, 4, 13, 12)])
def test_input_gradients_match_oracle(neurons, layers, C, lh):
    """dL/dpos and dL/ddir of one forward + backward against the oracle's autograd, the parameter gradients of the same run against the existing bar.
    4 tiles and a tail of 21, 5 positions outside the box; two shapes, because the workspace rows the kernel reads depend on W and NH.
    (On the parent commit `positions.grad is None`.)"""
    sc = H.make_scene(neurons=neurons, layers=layers, C=C, log2_hashmap_size=lh)
    hip, orc = H.hip_field(sc).train(), H.oracle_field(sc, requires_grad=True)
    pos, d, g = _samples(sc, 4 * 64 + 21, seed=11)
    p, q, outs = _hip_input_grads(hip, pos, d, g)
    assert p.grad is not None and q.grad is not None
    r_pos, r_dir = _oracle_input_grads(orc, pos, d, g)
    print(f"max |dL/dpos| {r_pos.abs().max():.3e}, max |dL/ddir| {r_dir.abs().max():.3e}")
    _close(p.grad, r_pos, "d_pos")
    _close(q.grad, r_dir, "d_dir")
    _close(p.grad[:5], r_pos[:5], "d_pos outside the box")
    n_mlp = sum(o * i for o, i in orc.shapes["base"])
    _close(hip.mlp_base.params.grad[:n_mlp], orc.p_base.grad[:n_mlp], "base mlp")
    _close(hip.mlp_base.params.grad[n_mlp:], orc.p_base.grad[n_mlp:], "hash table")
    _close(hip.mlp_head.params.grad, orc.p_head.grad, "rgb head")
    _close(hip.mlp_sem.params.grad, orc.p_sem.grad, "sem head")


# ------------------------------------------------------------------ 2. frozen parameters
def test_frozen_parameters_still_give_input_gradients():
    sc = H.make_scene(neurons=128, layers=2, C=29, log2_hashmap_size=14)
    hip, orc = H.hip_field(sc).train(), H.oracle_field(sc)
    for prm in hip.parameters():
        prm.requires_grad_(False)
    pos, d, g = _samples(sc, 150, seed=12)
    p, q, outs = _hip_input_grads(hip, pos, d, g)
    assert outs[0].requires_grad
    r_pos, r_dir = _oracle_input_grads(orc, pos, d, g)
    _close(p.grad, r_pos, "d_pos (frozen parameters)")
    _close(q.grad, r_dir, "d_dir (frozen parameters)")
    assert all(prm.grad is None for prm in hip.parameters())


# ------------------------------------------------------------------ 3. only what is asked
def _input_grad_launches(fn):
    lib = L.load_library()
    lib.mnf_profile_begin()
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        lib.mnf_profile_end(None, None)
    ms, cnt = ctypes.c_double(), ctypes.c_int64()
    lib.mnf_profile_query(b"field_input_grad", ctypes.byref(ms), ctypes.byref(cnt))
    dg = ctypes.c_int64()
    lib.mnf_profile_query(b"dgrad", None, ctypes.byref(dg))
    return cnt.value, dg.value


def test_only_the_gradients_asked_for():
    sc = H.make_scene(neurons=64, layers=2, C=5, log2_hashmap_size=12)
    hip, orc = H.hip_field(sc).train(), H.oracle_field(sc)
    pos, d, g = _samples(sc, 150, seed=13)
    p, q, _ = _hip_input_grads(hip, pos, d, g, pos_grad=False)
    assert p.grad is None and q.grad is not None
    _close(q.grad, _oracle_input_grads(orc, pos, d, g)[1], "d_dir alone")
    none, dgrad = _input_grad_launches(lambda: _hip_input_grads(hip, pos, d, g, pos_grad=False, dir_grad=False))
    assert none == 0 and dgrad == 1, (none, dgrad)          # a forward and a backward ran, the input-gradient kernel did not
    both, dgrad = _input_grad_launches(lambda: _hip_input_grads(hip, pos, d, g))
    assert both == 1 and dgrad == 1, (both, dgrad)


# ------------------------------------------------------------------ 4. precision modes
@pytest.mark.parametrize("mode", ["mfma_bf16", "blend_fp16", "output_fp16"])
def test_input_gradients_in_other_modes(mode):
    field_kw = dict(mfma_bf16=mode == "mfma_bf16", tcnn_blend_fp16=mode == "blend_fp16", tcnn_output_rounding=mode == "output_fp16")
    oracle_kw = dict(precision="bf16" if mode == "mfma_bf16" else "f16", blend="f16" if mode == "blend_fp16" else "f32",
                     output_rounding=mode == "output_fp16")
    bar = BF16_BAR if mode == "mfma_bf16" else F16_BAR
    sc = H.make_scene(neurons=128, layers=2, C=29, log2_hashmap_size=14)
    hip, orc = H.hip_field(sc, **field_kw).train(), H.oracle_field(sc, **oracle_kw)
    pos, d, g = _samples(sc, 150, seed=14)
    p, q, _ = _hip_input_grads(hip, pos, d, g)
    r_pos, r_dir = _oracle_input_grads(orc, pos, d, g)
    _close(p.grad, r_pos, f"d_pos ({mode})", **bar)
    _close(q.grad, r_dir, f"d_dir ({mode})", **bar)


# ------------------------------------------------------------------ 5. rays
@pytest.fixture(scope="module")
def view():
    """64 rays of an 8 x 8 view of a small scene and their sample set from the HIP estimator (eval mode: no jitter), shared by the ray tests"""
    from apnrf_amd.ngp import RaySigmaFn
    sc = H.make_scene(neurons=64, layers=2, C=5, log2_hashmap_size=12)
    hip, est = H.hip_field(sc), H.hip_estimator(sc)
    o, d = H.view_rays(sc, 1, h=8, w=8)
    o, d = o.float().contiguous(), d.float().contiguous()
    ri, ts, te = est.sampling(o.to(DEV), d.to(DEV), sigma_fn=RaySigmaFn(hip, o.to(DEV), d.to(DEV)), stratified=False, **H.RENDER_KW)
    return dict(sc=sc, hip=hip, est=est, o=o, d=d, ri=ri, ts=ts, te=te)


def test_ray_gradients_match_oracle(view):
    from apnrf_amd import render as RD
    from oracle import render as R
    sc, hip = view["sc"], view["hip"]
    orc = H.oracle_field(sc)
    a = torch.from_numpy(sc["aabb"])
    away_d = torch.nn.functional.normalize(torch.tensor([[1.0, 0.5, 0.25]]) + 0.1 * torch.arange(8)[:, None], dim=-1)
    o = torch.cat([view["o"], (a[3:] + 1.0).expand(8, 3)]).contiguous()        # 8 rays outside the box, pointing away from it: no samples
    d = torch.cat([view["d"], away_d]).contiguous()
    ri, ts, te = view["ri"], view["ts"], view["te"]
    n_rays, C = o.shape[0], sc["C"]
    rng = np.random.default_rng(15)
    cot = [(rng.normal(size=(n_rays, k)) * 1e-3).astype(np.float32) for k in (3, 1, 1, C)]
    ro, rd = o.to(DEV).requires_grad_(), d.to(DEV).requires_grad_()
    outs = RD.sem_rendering(hip, RD.Rays(ro, rd), ts, te, ri, n_rays)[:4]
    torch.autograd.backward(list(outs), [_cu(c) for c in cot])
    co, cd = o.clone().requires_grad_(), d.clone().requires_grad_()
    ref = R.sem_rendering(orc, co, cd, ts.cpu(), te.cpu(), ri.cpu(), n_rays)[:4]
    for name, x, y in zip(("rgb", "acc", "depth", "sem"), outs, ref):
        np.testing.assert_allclose(x.detach().cpu().numpy(), y.detach().numpy(), atol=1e-3, rtol=1e-3, err_msg=name)
    torch.autograd.backward(list(ref), [torch.from_numpy(c) for c in cot])
    nonzero = int((co.grad[:64].abs().sum(-1) > 0).sum())
    print(f"{ts.shape[0]} kept samples, ray gradients non-zero on {nonzero} of 64 rays")
    assert nonzero > 32
    _close(ro.grad, co.grad, "g_o")
    _close(rd.grad, cd.grad, "g_d")
    assert bool((ro.grad[64:] == 0).all()) and bool((rd.grad[64:] == 0).all())
    assert bool((co.grad[64:] == 0).all()) and bool((cd.grad[64:] == 0).all())


# ------------------------------------------------------------------ 6. the ray kernel alone
def test_ray_input_gradients_kernel():
    """g_o = sum d_pos, g_d = sum (t_mid d_pos + d_dir) per chunk against float64 sums.  Bound per component, derived: the kernel adds the cnt values
    of a chunk in fp32 in some fixed order (at most cnt - 1 roundings on any path, each relative 2^-24 of a partial sum that is at most sum |terms|), and
    forms each term with at most three more roundings (t_start + t_end, the product, the addition of d_dir; the halving is exact), each relative 2^-24
    of |t_mid d_pos| or |d_dir|: |got - ref| <= (cnt + 2) 2^-24 sum |terms| to first order, asserted with the factor 2 of headroom the issue states,
    (cnt + 2) 2^-23 sum |terms|, where the terms of g_d are the addends t_mid d_pos[s] and d_dir[s]."""
    lib = L.load_library()
    rng = np.random.default_rng(16)
    cnts = np.array([0, 1, 63, 64, 65, 700], np.int64)
    starts = np.concatenate([[0], np.cumsum(cnts)[:-1]]).astype(np.int64)
    n = int(cnts.sum())
    dp, dd = rng.normal(size=(n, 3)).astype(np.float32), rng.normal(size=(n, 3)).astype(np.float32)
    t0 = (rng.random(n) * 5).astype(np.float32); t1 = (t0 + rng.random(n).astype(np.float32) * 0.01).astype(np.float32)
    tm = (t0.astype(np.float64) + t1.astype(np.float64)) / 2
    args = [_cu(x) for x in (dp, dd, t0, t1, starts, cnts)]
    for with_dir in (True, False):
        g_o, g_d = torch.full((len(cnts), 3), 7.0, device=DEV), torch.full((len(cnts), 3), 7.0, device=DEV)
        L.launch(lib.mnf_ray_input_gradients, L.ptr(args[0]), L.ptr(args[1]) if with_dir else None, L.ptr(args[2]), L.ptr(args[3]), L.ptr(args[4]),
                 L.ptr(args[5]), len(cnts), n, L.ptr(g_o), L.ptr(g_d))
        g_o, g_d = g_o.cpu().numpy().astype(np.float64), g_d.cpu().numpy().astype(np.float64)
        for r, (s, c) in enumerate(zip(starts, cnts)):
            sl = slice(s, s + c)
            t_pos = tm[sl, None] * dp[sl].astype(np.float64)
            t_dir = dd[sl].astype(np.float64) if with_dir else np.zeros_like(t_pos)
            ref_o, ref_d = dp[sl].astype(np.float64).sum(0), (t_pos + t_dir).sum(0)
            bound_o = (c + 2) * 2.0 ** -23 * np.abs(dp[sl].astype(np.float64)).sum(0)
            bound_d = (c + 2) * 2.0 ** -23 * (np.abs(t_pos) + np.abs(t_dir)).sum(0)
            print(f"chunk of {c} (d_dir {with_dir}): |g_o err| {np.abs(g_o[r] - ref_o).max():.2e} (bound {bound_o.min():.2e}), "
                  f"|g_d err| {np.abs(g_d[r] - ref_d).max():.2e} (bound {bound_d.min():.2e})")
            assert (np.abs(g_o[r] - ref_o) <= bound_o).all() and (np.abs(g_d[r] - ref_d) <= bound_d).all(), (r, c)
        assert (g_o[0] == 0).all() and (g_d[0] == 0).all()          # the empty chunk: exact zeros, written


# ------------------------------------------------------------------ 7. same workspace, same bits; 10. arguments
def _c_abi_case(n, with_backward):
    """A handle, the inputs of one train forward (+ backward) through the C ABI, and a call of `mnf_field_backward_inputs` on its workspace"""
    lib = L.load_library()
    sc = H.make_scene(neurons=64, layers=2, C=5, log2_hashmap_size=12)
    hip = H.hip_field(sc)
    h = hip._ensure_handle()
    pos, d, g = _samples(sc, max(n, 1), seed=17)
    pos, d = _cu(pos), _cu(d)
    nbytes = int(lib.mnf_field_train_workspace_bytes(h, n))
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
    if with_backward:
        rgb, sigma, sem = torch.empty(n, 3, device=DEV), torch.empty(n, 1, device=DEV), torch.empty(n, sc["C"], device=DEV)
        L.launch(lib.mnf_field_forward_train, h, L.ptr(pos), L.ptr(d), n, L.ptr(rgb), L.ptr(sigma), L.ptr(sem), L.ptr(ws), nbytes)
        grads = [torch.empty_like(prm) for prm in (hip.mlp_base.params, hip.mlp_head.params, hip.mlp_sem.params)]
        gs = [_cu(x) for x in g]
        L.launch(lib.mnf_field_backward, h, L.ptr(pos), n, L.ptr(gs[0]), L.ptr(gs[1]), L.ptr(gs[2]), L.ptr(rgb), L.ptr(sigma), L.ptr(ws), nbytes, 128.0,
                 L.ptr(grads[0]), L.ptr(grads[1]), L.ptr(grads[2]))

    def call(n_=n, ws_=ws, nbytes_=nbytes, scale=128.0, out_pos=True, out_dir=True, dirs=True):
        d_pos, d_dir = torch.full((max(n, 1), 3), 7.0, device=DEV), torch.full((max(n, 1), 3), 7.0, device=DEV)
        rc = lib.mnf_field_backward_inputs(h, L.ptr(pos), L.ptr(d) if dirs else None, n_, L.ptr(ws_) if ws_ is not None else None, nbytes_, scale,
                                           L.ptr(d_pos) if out_pos else None, L.ptr(d_dir) if out_dir else None, L.stream())
        torch.cuda.synchronize()
        return rc, d_pos, d_dir
    return hip, call, nbytes


def test_same_workspace_same_bits():
    hip, call, _ = _c_abi_case(4 * 64 + 21, with_backward=True)
    rc1, p1, q1 = call()
    rc2, p2, q2 = call()
    assert rc1 == 0 and rc2 == 0
    assert bool((p1 != 7.0).any()) and bool((q1 != 7.0).any())
    assert torch.equal(p1, p2) and torch.equal(q1, q2)
    rc3, p3, _ = call(out_dir=False, dirs=False)                    # positions alone, directions NULL: the same position gradient
    assert rc3 == 0 and torch.equal(p1, p3)


def test_argument_errors_enqueue_nothing():
    n = 100
    hip, call, nbytes = _c_abi_case(n, with_backward=False)
    INVALID, WORKSPACE = -1, -4
    cases = [("both outputs NULL", dict(out_pos=False, out_dir=False), INVALID), ("n < 0", dict(n_=-1), INVALID),
             ("loss_scale 0", dict(scale=0.0), INVALID), ("loss_scale < 0", dict(scale=-128.0), INVALID),
             ("d_directions without directions", dict(dirs=False), INVALID),
             ("workspace one byte short", dict(nbytes_=nbytes - 1), WORKSPACE), ("workspace NULL", dict(ws_=None), WORKSPACE),
             ("n == 0", dict(n_=0), 0), ("n == 0 without a workspace", dict(n_=0, ws_=None, nbytes_=0), 0)]

    def run():
        for name, kw, want in cases:
            rc, d_pos, d_dir = call(**kw)
            assert rc == want, (name, rc, L.load_library().mnf_last_error())
            assert bool((d_pos == 7.0).all()) and bool((d_dir == 7.0).all()), name      # nothing was written
    launches, _ = _input_grad_launches(run)
    assert launches == 0


# ------------------------------------------------------------------ 8. the pose vector
def test_pose_vector_gradient_matches_oracle(view):
    """d(L2 photometric loss against the un-perturbed render)/d(rotvec, trans) through `transform_rays` and the drop-in `sem_rendering` with frozen
    parameters, against the same chain through the oracle (built here from oracle.render.sem_rendering: render_train takes numpy rays).  Each side's
    target is its own un-perturbed render of the same sample set."""
    from apnrf_amd import render as RD
    from oracle import render as R
    sc, hip = view["sc"], view["hip"]
    orc = H.oracle_field(sc)
    ri, ts, te, n_rays = view["ri"], view["ts"], view["te"], view["o"].shape[0]
    xi = np.array([0.01, -0.02, 0.015, 0.02, -0.01, 0.015], np.float32)
    hip.zero_grad(set_to_none=True)                                 # (the fixture's field is shared: an earlier test left parameter gradients)
    for prm in hip.parameters():
        prm.requires_grad_(False)
    try:
        with torch.no_grad():
            target = RD.sem_rendering(hip, RD.Rays(view["o"].to(DEV), view["d"].to(DEV)), ts, te, ri, n_rays)[0]
        rot, tr = _cu(xi[:3]).requires_grad_(), _cu(xi[3:]).requires_grad_()
        rays = RD.transform_rays(RD.Rays(view["o"].to(DEV), view["d"].to(DEV)), rot, tr)
        rgb = RD.sem_rendering(hip, rays, ts, te, ri, n_rays)[0]
        loss = ((rgb - target) ** 2).mean()
        loss.backward()
        assert all(prm.grad is None for prm in hip.parameters())
    finally:
        for prm in hip.parameters():
            prm.requires_grad_(True)
    with torch.no_grad():
        r_target = R.sem_rendering(orc, view["o"], view["d"], ts.cpu(), te.cpu(), ri.cpu(), n_rays)[0]
    r_rot, r_tr = torch.from_numpy(xi[:3].copy()).requires_grad_(), torch.from_numpy(xi[3:].copy()).requires_grad_()
    r_rays = RD.transform_rays(RD.Rays(view["o"], view["d"]), r_rot, r_tr)                 # pure torch: the same transform on the CPU
    r_rgb = R.sem_rendering(orc, r_rays.origins, r_rays.viewdirs, ts.cpu(), te.cpu(), ri.cpu(), n_rays)[0]
    r_loss = ((r_rgb - r_target) ** 2).mean()
    r_loss.backward()
    got, want = torch.cat([rot.grad, tr.grad]).cpu(), torch.cat([r_rot.grad, r_tr.grad])
    err, c = _figures(got, want)
    print(f"loss {loss.item():.4e} (oracle {r_loss.item():.4e}); pose gradient {got.numpy()} vs {want.numpy()}: rel L2 {err:.3e}, cos {c:.6f}")
    assert err < 2e-2, err


def test_transform_rays_at_zero_and_against_a_rotation_matrix():
    """identity at zero with a finite gradient (the series branch); at a finite angle the Rodrigues matrix of the axis and angle (pure torch, on the device)"""
    from apnrf_amd import render as RD
    o = torch.tensor([[1.0, 2.0, 3.0]], device=DEV).expand(5, 3).contiguous()
    d = torch.nn.functional.normalize(torch.arange(15.0, device=DEV).reshape(5, 3) - 7.0, dim=-1)
    rot, tr = torch.zeros(3, device=DEV, requires_grad=True), torch.zeros(3, device=DEV, requires_grad=True)
    r = RD.transform_rays(RD.Rays(o, d), rot, tr)
    assert torch.equal(r.origins, o) and torch.allclose(r.viewdirs, d, atol=1e-7)
    (r.viewdirs * torch.arange(15.0, device=DEV).reshape(5, 3)).sum().backward()
    assert bool(torch.isfinite(rot.grad).all()) and bool((rot.grad != 0).any())
    ang = 0.7
    r = RD.transform_rays(RD.Rays(o, d), torch.tensor([0.0, ang, 0.0], device=DEV), torch.tensor([0.5, 0.0, -1.0], device=DEV))
    Ry = torch.tensor([[np.cos(ang), 0.0, np.sin(ang)], [0.0, 1.0, 0.0], [-np.sin(ang), 0.0, np.cos(ang)]], dtype=torch.float32, device=DEV)
    assert torch.allclose(r.viewdirs, d @ Ry.T, atol=1e-6)
    assert torch.allclose(r.origins, o + torch.tensor([0.5, 0.0, -1.0], device=DEV), atol=1e-6)      # a common origin only moves by the translation


# ------------------------------------------------------------------ 9. the fused route
def test_fused_train_render_hands_over_for_ray_gradients(view):
    from apnrf_amd import render as RD
    hip, est = view["hip"], view["est"]
    assert not hip.training
    bk = torch.tensor([0.5, 0.2, 0.9], device=DEV)
    o1, d1 = view["o"].to(DEV).requires_grad_(), view["d"].to(DEV).requires_grad_()
    out = RD.fused_train_render(hip, est, RD.Rays(o1, d1), render_bkgd=bk, **H.RENDER_KW)
    assert RD.latest_train_render(hip) is None                      # handed over
    o2, d2 = view["o"].to(DEV).requires_grad_(), view["d"].to(DEV).requires_grad_()
    ref = RD.render_image_with_occgrid_with_depth_guide(hip, est, RD.Rays(o2, d2), render_bkgd=bk, **H.RENDER_KW)
    assert out[4] == ref[4] and out[4] > 100
    for x, y in zip(out[:4], ref[:4]):
        assert torch.equal(x, y)
    (out[0].sum() + out[3].sum()).backward()
    assert o1.grad is not None and d1.grad is not None and bool((o1.grad != 0).any()) and bool((d1.grad != 0).any())
    hip.zero_grad()
    RD.fused_train_render(hip, est, RD.Rays(view["o"].to(DEV), view["d"].to(DEV)), render_bkgd=bk, **H.RENDER_KW)
    assert RD.latest_train_render(hip) is not None                  # without the flag on the rays: the fused kernels, as before
