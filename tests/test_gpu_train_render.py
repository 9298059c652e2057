"""GPU tests of the differentiable fused train render: `render.fused_train_render` (`mnf_train_render_forward` / `mnf_train_render_backward`, the one-call
train step cut at its loss) against the oracle's autograd and against the one-call step itself.  Bars are the project's own: rendered rgb / acc / depth 1e-3
absolute, class logits max(1e-3, 3e-4 x the ray's largest |logit|), loss against the oracle rtol 1e-4, loss between two routes of the
product rtol 2e-5, gradient groups `_grad_close` at rel 3e-2 / cosine 0.999; bf16: 8x the value bars, gradients at the bf16 bars of test_gpu_precision_modes
(rel 6e-2, cosine 0.998).  Batches: 182 rays of a sub-sampled view plus 11 rays that miss the box = 193 (no multiple of 64)."""
import functools

import numpy as np
import pytest
import torch

import helpers as H
from test_gpu_parity import _grad_close

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BK = torch.tensor([0.5, 0.2, 0.9])
N_MISS = 11


def _loss(rgb, depth, sem, pix, dep, lab):
    import torch.nn.functional as F
    return F.smooth_l1_loss(rgb, pix) * 10 + F.smooth_l1_loss(depth, dep.unsqueeze(1)) / 5 + F.cross_entropy(sem, lab) / 2      # pipeline.py:506-511


def _loss7(rgb, acc, depth, sem, pix, dep, lab):      # the same loss with `train_step(loss_fn=...)`'s signature
    return _loss(rgb, depth, sem, pix, dep, lab)


def _masked_loss(rgb, acc, depth, pix, dep):
    """A loss the one-call step cannot express: L2 on rgb + 0.1 mean|acc - 1| + L1 on depth only where the target depth > 1.0; the class logits unused."""
    m = dep > 1.0
    return ((rgb - pix) ** 2).mean() + 0.1 * (acc - 1.0).abs().mean() + (depth[:, 0] - dep)[m].abs().sum() / m.sum()


def _targets(n, C, seed=3):
    rng = np.random.default_rng(seed)
    return (torch.from_numpy(rng.random((n, 3)).astype(np.float32)), torch.from_numpy(rng.uniform(0.5, 4.0, n).astype(np.float32)),
            torch.from_numpy(rng.integers(0, C, n)))


def _with_misses(sc, o, d):
    """N_MISS rays appended that start beyond the box and look away from it"""
    far = torch.from_numpy(sc["aabb"][3:]) + 5.0
    return torch.cat([o, far.expand(N_MISS, 3)], 0).contiguous(), torch.cat([d, torch.tensor([0.0, 1.0, 0.0]).expand(N_MISS, 3)], 0).contiguous()


@functools.lru_cache(maxsize=None)
def _case(neurons=128, layers=2, C=29, bf16=False, pose=4):
    """One batch of one model and the oracle's train render of it (computed once, shared, never written to: gradients come from `torch.autograd.grad`)."""
    from oracle import render as R
    sc = H.make_scene(neurons=neurons, layers=layers, C=C, log2_hashmap_size=15)
    o, d = _with_misses(sc, *H.view_rays(sc, pose, h=13, w=14))
    n = o.shape[0]
    orc = H.oracle_field(sc, precision="bf16" if bf16 else "f16", requires_grad=True)
    est = H.hip_estimator(sc)
    ref = R.render_train(orc, sc["occ"], est.aabbs.cpu().numpy(), float(est.occs.mean().item()), o, d, torch.full((n,), 0.1), render_bkgd=BK,
                         render_step_size=1e-3, cone_angle=0.004, alpha_thre=0.01)
    pix, dep, lab = _targets(n, C)
    return dict(sc=sc, o=o, d=d, n=n, orc=orc, est=est, ref=ref, pix=pix, dep=dep, lab=lab, field_kw=dict(mfma_bf16=bf16))


def _rays(case):
    from apnrf_amd import render as RD
    return RD.Rays(case["o"].to(DEV), case["d"].to(DEV))


def _params(f):
    return [f.mlp_base.params, f.mlp_head.params, f.mlp_sem.params]


def _check_planes(got, ref, tol=1.0):
    rgb, acc, depth, sem = (t.detach().cpu() for t in got)
    for name, g, w in (("rgb", rgb, ref[0]), ("acc", acc, ref[1]), ("depth", depth, ref[2])):
        err = float((g - w.detach()).abs().max())
        print(f"train render {name}: max abs err vs oracle {err:.3e}")
        assert err < 1e-3 * tol, (name, err)
    want = ref[3].detach()
    bar = torch.clamp(3e-4 * want.abs().max(dim=1, keepdim=True).values, min=1e-3) * tol
    ratio = float(((sem - want).abs() / bar).max())
    print(f"train render sem: max err / bar {ratio:.3f}")
    assert ratio < 1.0, ratio


def _check_grads(got, orc, want, rel=3e-2, cos=0.999, sem=True):
    n_mlp = sum(o_ * i_ for o_, i_ in orc.shapes["base"])
    _grad_close(got[0][:n_mlp], want[0][:n_mlp], "base mlp", rel=rel, cos=cos)
    _grad_close(got[0][n_mlp:], want[0][n_mlp:], "hash table", rel=rel, cos=cos)
    _grad_close(got[1], want[1], "rgb head", rel=rel, cos=cos)
    if sem:
        _grad_close(got[2], want[2], "sem head", rel=rel, cos=cos)


def _oracle_grads(case, loss):
    orc = case["orc"]
    return torch.autograd.grad(loss, [orc.p_base, orc.p_head, orc.p_sem], retain_graph=True, allow_unused=True)


# ------------------------------------------------------------------ 1. forward
def test_forward_matches_oracle_one_level():
    """Outputs and sample count against `oracle.render.render_train`: the count exactly, and equal to `fused_forward_backward`'s on the same batch; the rays that
    miss the box come out as background / zeros; the drop-in's shapes for [H, W, 3] rays."""
    from apnrf_amd import render as RD
    c = _case()
    hip = H.hip_field(c["sc"]).train()
    rays = _rays(c)
    rgb, acc, depth, sem, n = RD.fused_train_render(hip, c["est"], rays, render_bkgd=BK.to(DEV), stratified=False, **H.RENDER_KW)
    assert isinstance(n, int) and n == c["ref"][4] and n > 500
    assert rgb.shape == (c["n"], 3) and acc.shape == (c["n"], 1) and depth.shape == (c["n"], 1) and sem.shape == (c["n"], 29)
    assert rgb.requires_grad and sem.requires_grad
    _check_planes((rgb, acc, depth, sem), c["ref"])
    assert torch.equal(rgb[-N_MISS:].detach().cpu(), BK.expand(N_MISS, 3)) and float(acc[-N_MISS:].abs().max()) == 0.0
    assert float(depth[-N_MISS:].abs().max()) == 0.0 and float(sem[-N_MISS:].abs().max()) == 0.0
    pix, dep, lab = (t.to(DEV) for t in (c["pix"], c["dep"], c["lab"]))
    step = RD.fused_forward_backward(H.hip_field(c["sc"]).train(), c["est"], rays, pix, dep, lab, BK.to(DEV), stratified=False, **H.RENDER_KW)
    assert step["n_rendering_samples"] == n
    last = RD.latest_train_render(hip)
    assert last["counts"].tolist()[:2] == [step["n_marched"], n] and int(last["counts"][3]) == 0 and int(last["skip"]) == 0
    with torch.no_grad():      # nothing kept for a backward; leading shape [2, 91] as the drop-in reshapes it
        img = RD.Rays(rays.origins[:182].view(2, 91, 3), rays.viewdirs[:182].view(2, 91, 3))
        out = RD.fused_train_render(hip, c["est"], img, render_bkgd=BK.to(DEV), stratified=False, **H.RENDER_KW)
    assert out[0].shape == (2, 91, 3) and out[1].shape == (2, 91, 1) and out[3].shape == (2, 91, 29) and not out[0].requires_grad
    assert all(bool(torch.isfinite(t).all()) for t in out[:4]) and out[4] == n


def test_forward_matches_oracle_two_occupancy_levels():
    from apnrf_amd import render as RD
    from oracle import render as R
    from test_gpu_round3 import _multi_level_estimator
    sc = H.make_scene(log2_hashmap_size=15, seed=6)
    est, occ = _multi_level_estimator(2)
    fs = dict(sc); fs["aabb"] = est.aabbs[-1].cpu().numpy().astype(np.float32)      # the field covers the outer level's box
    o, d = H.view_rays(sc, 3, h=13, w=14)
    o, d = _with_misses(fs, o + torch.tensor([3.0, 0.0, 3.0]), d)
    n = o.shape[0]
    hip, orc = H.hip_field(fs).train(), H.oracle_field(fs)
    rays = RD.Rays(o.to(DEV), d.to(DEV))
    got = RD.fused_train_render(hip, est, rays, render_bkgd=BK.to(DEV), stratified=False, **H.RENDER_KW)
    ref = R.render_train(orc, occ, est.aabbs.cpu().numpy(), float(est.occs.mean().item()), o, d, torch.full((n,), 0.1), render_bkgd=BK, render_step_size=1e-3,
                         cone_angle=0.004, alpha_thre=0.01)
    assert got[4] == ref[4] and got[4] > 500
    _check_planes(got[:4], ref)
    pix, dep, lab = (t.to(DEV) for t in _targets(n, 29))
    step = RD.fused_forward_backward(H.hip_field(fs).train(), est, rays, pix, dep, lab, BK.to(DEV), stratified=False, **H.RENDER_KW)
    assert step["n_rendering_samples"] == got[4]


# ------------------------------------------------------------------ 2. the reference's loss lines kept in torch
@pytest.mark.parametrize("neurons,layers,bf16", [(64, 4, False), (128, 2, True)])
def test_reference_loss_in_torch_matches_oracle_and_one_call_step(neurons, layers, bf16):
    from apnrf_amd import render as RD
    c = _case(neurons, layers, 29, bf16)
    tol = 8.0 if bf16 else 1.0
    hip = H.hip_field(c["sc"], **c["field_kw"]).train()
    rays = _rays(c)
    pix, dep, lab = (t.to(DEV) for t in (c["pix"], c["dep"], c["lab"]))
    rgb, acc, depth, sem, n = RD.fused_train_render(hip, c["est"], rays, render_bkgd=BK.to(DEV), stratified=False, **H.RENDER_KW)
    loss = _loss(rgb, depth, sem, pix, dep, lab)
    loss.backward()
    ref = c["ref"]
    r_loss = _loss(ref[0], ref[2], ref[3], c["pix"], c["dep"], c["lab"])
    assert n == ref[4]
    _check_planes((rgb, acc, depth, sem), ref, tol)
    print(f"reference loss {neurons}x{layers} bf16={bf16}: {float(loss):.6f} vs oracle {float(r_loss):.6f}")
    np.testing.assert_allclose(float(loss.detach()), float(r_loss.detach()), rtol=1e-4 * tol)
    _check_grads([p.grad for p in _params(hip)], c["orc"], _oracle_grads(c, r_loss), **(dict(rel=6e-2, cos=0.998) if bf16 else {}))
    other = H.hip_field(c["sc"], **c["field_kw"]).train()
    step = RD.fused_forward_backward(other, c["est"], rays, pix, dep, lab, BK.to(DEV), stratified=False, **H.RENDER_KW)
    assert step["n_rendering_samples"] == n
    np.testing.assert_allclose(float(loss.detach()), float(step["loss"]), rtol=2e-5)


# ------------------------------------------------------------------ 3. a loss the one-call step cannot express
def test_masked_depth_opacity_loss_matches_oracle_autograd():
    """First use of the opacity gradient inside the step's workspace and of a NULL gradient (the class logits are unused)."""
    from apnrf_amd import render as RD
    c = _case()
    hip = H.hip_field(c["sc"]).train()
    pix, dep = c["pix"].to(DEV), c["dep"].to(DEV)
    rgb, acc, depth, sem, n = RD.fused_train_render(hip, c["est"], _rays(c), render_bkgd=BK.to(DEV), stratified=False, **H.RENDER_KW)
    loss = _masked_loss(rgb, acc, depth, pix, dep)
    loss.backward()
    ref = c["ref"]
    r_loss = _masked_loss(ref[0], ref[1], ref[2], c["pix"], c["dep"])
    print(f"masked loss: {float(loss):.6f} vs oracle {float(r_loss):.6f}")
    np.testing.assert_allclose(float(loss.detach()), float(r_loss.detach()), rtol=1e-4)
    want = _oracle_grads(c, r_loss)
    assert want[2] is None or float(want[2].abs().max()) == 0.0
    _check_grads([p.grad for p in _params(hip)], c["orc"], want, sem=False)
    assert float(hip.mlp_sem.params.grad.abs().max()) == 0.0
    last = RD.latest_train_render(hip)
    assert int(last["skip"]) == 0 and int(last["counts"][3]) == 0


# ------------------------------------------------------------------ 4. strides
def _grads_of(hip, c, loss_of):
    from apnrf_amd import render as RD
    planes = RD.fused_train_render(hip, c["est"], _rays(c), render_bkgd=BK.to(DEV), stratified=False, deterministic=True, **H.RENDER_KW)
    return torch.autograd.grad(loss_of(*planes[:4]), _params(hip))


def test_expanded_and_transposed_gradients_equal_their_contiguous_forms(monkeypatch):
    """`rgb.mean() + depth.sum()` hands the backward expanded stride-0 gradients, a loss on `sem.t()` a transposed view: both give the bits of the same loss
    written with materialised contiguous weights (deterministic accumulation).  The strides and NULL pointers `mnf_train_render_backward` is given are logged."""
    from apnrf_amd import _lib as L
    c = _case()
    hip = H.hip_field(c["sc"]).train()
    R_ = c["n"]
    seen, launch, entry = [], L.launch, L.load_library().mnf_train_render_backward

    def spy(fn, *a, **k):
        if fn is entry:      # (handle, R, opts, g_rgb, rs, cs, g_acc, rs, g_depth, rs, g_sem, rs, cs, ...)
            seen.append(dict(rgb=a[3] and (a[4], a[5]), acc=a[6] and a[7], depth=a[8] and a[9], sem=a[10] and (a[11], a[12])))
        return launch(fn, *a, **k)
    monkeypatch.setattr(L, "launch", spy)
    w_rgb = torch.ones(R_, 3, device=DEV) / (3 * R_)
    w_dep = torch.ones(R_, 1, device=DEV)
    a = _grads_of(hip, c, lambda rgb, acc, depth, sem: rgb.mean() + depth.sum())
    b = _grads_of(hip, c, lambda rgb, acc, depth, sem: (rgb * w_rgb).sum() + (depth * w_dep).sum())
    print("strides handed to the backward:", seen)
    # (`sum` hands over an expanded scalar; whether `mean`'s division materialises its expansion is torch's choice: both forms are read through their strides)
    assert seen[0]["depth"] == 0 and seen[0]["rgb"] in ((0, 0), (3, 1)) and seen[0]["acc"] is None and seen[0]["sem"] is None
    assert seen[1] == dict(rgb=(3, 1), acc=None, depth=1, sem=None)
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and float(a[0].abs().max()) > 0
    wt = torch.from_numpy(np.random.default_rng(5).normal(size=(29, R_)).astype(np.float32)).to(DEV)
    w_dense = wt.t().contiguous()
    a = _grads_of(hip, c, lambda rgb, acc, depth, sem: (sem.t() * wt).sum())
    b = _grads_of(hip, c, lambda rgb, acc, depth, sem: (sem * w_dense).sum())
    assert seen[2] == dict(rgb=None, acc=None, depth=None, sem=(1, R_)) and seen[3] == dict(rgb=None, acc=None, depth=None, sem=(29, 1))
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and float(a[2].abs().max()) > 0


def test_dense_gradients_off_the_16_byte_boundary_equal_the_aligned_ones():
    """Dense gradients that start 4, 8 and 12 bytes behind a 16-byte boundary (views into a larger buffer, handed over as `grad_outputs`) are read with a
    scalar head, 16-byte loads and a scalar tail: the bits of the same values in tensors of their own."""
    from apnrf_amd import render as RD
    c = _case()
    hip = H.hip_field(c["sc"]).train()
    R_, rng = c["n"], np.random.default_rng(9)
    vals = [torch.from_numpy(rng.normal(size=(R_, k)).astype(np.float32)).to(DEV) for k in (3, 1, 1, 29)]

    def grads(outs):
        planes = RD.fused_train_render(hip, c["est"], _rays(c), render_bkgd=BK.to(DEV), stratified=False, deterministic=True, **H.RENDER_KW)
        return torch.autograd.grad(planes[:4], _params(hip), grad_outputs=outs)
    want = grads(vals)
    assert all(v.data_ptr() % 16 == 0 for v in vals) and float(want[0].abs().max()) > 0
    for off in (1, 2, 3):
        shifted = []
        for v in vals:
            buf = torch.zeros(v.numel() + 8, device=DEV)
            buf[off:off + v.numel()] = v.reshape(-1)
            shifted.append(buf[off:off + v.numel()].view(v.shape))
        assert all(x.data_ptr() % 16 == 4 * off and x.is_contiguous() for x in shifted)
        got = grads(shifted)
        assert all(torch.equal(x, y) for x, y in zip(got, want)), off


# ------------------------------------------------------------------ 5. bounds
def test_render_beyond_its_bounds_is_repeated_with_larger_ones(monkeypatch):
    from apnrf_amd import render as RD
    c = _case()
    rays = _rays(c)
    kw = dict(render_bkgd=BK.to(DEV), stratified=False, deterministic=True, **H.RENDER_KW)
    want = RD.fused_train_render(H.hip_field(c["sc"]).train(), c["est"], rays, **kw)
    statuses = []
    launch = RD._launch_train_render

    def logged(*a, **k):
        out = launch(*a, **k)
        statuses.append(int(out["counts"][3]))
        return out
    monkeypatch.setattr(RD, "_launch_train_render", logged)
    monkeypatch.setattr(RD.TrainState, "_own", lambda self, R: self.by_R.get(R, (256, 128)))
    hip = H.hip_field(c["sc"]).train()
    got = RD.fused_train_render(hip, c["est"], rays, **kw)
    print("bounds: statuses of the attempts", statuses)
    assert len(statuses) >= 2 and statuses[0] & 5 and statuses[-1] == 0
    assert got[4] == want[4] and all(torch.equal(g, w) for g, w in zip(got[:4], want[:4]))
    grads = torch.autograd.grad(got[0].sum() + got[3].sum(), _params(hip))
    assert all(bool(torch.isfinite(g).all()) for g in grads) and float(grads[0].abs().max()) > 0


# ------------------------------------------------------------------ 6. interleaving
def test_two_renders_of_one_field_interleave():
    """forward A, forward B, backward B, backward A on one field (different rays, a workspace each): each gradient has the bits of A and B run one after the
    other — every bit of per-call state lives in the call's workspace, the deterministic mode's scratch on the handle is only touched inside a backward."""
    from apnrf_amd import render as RD
    ca, cb = _case(), None
    sc = ca["sc"]
    ob, db = _with_misses(sc, *H.view_rays(sc, 2, h=13, w=14))
    rays_a, rays_b = _rays(ca), RD.Rays(ob.to(DEV), db.to(DEV))
    pix, dep, lab = (t.to(DEV) for t in (ca["pix"], ca["dep"], ca["lab"]))
    kw = dict(render_bkgd=BK.to(DEV), stratified=False, deterministic=True, **H.RENDER_KW)
    loss_of = lambda p: _loss(p[0], p[2], p[3], pix, dep, lab)
    hip = H.hip_field(sc).train()
    seq_a = torch.autograd.grad(loss_of(RD.fused_train_render(hip, ca["est"], rays_a, **kw)), _params(hip))
    seq_b = torch.autograd.grad(loss_of(RD.fused_train_render(hip, ca["est"], rays_b, **kw)), _params(hip))
    pa = RD.fused_train_render(hip, ca["est"], rays_a, **kw)
    pb = RD.fused_train_render(hip, ca["est"], rays_b, **kw)
    assert pa[4] != pb[4]
    int_b = torch.autograd.grad(loss_of(pb), _params(hip))
    int_a = torch.autograd.grad(loss_of(pa), _params(hip))
    assert all(torch.equal(x, y) for x, y in zip(int_a, seq_a)) and all(torch.equal(x, y) for x, y in zip(int_b, seq_b))
    assert not torch.equal(seq_a[0], seq_b[0])


# ------------------------------------------------------------------ 7. nothing to render
@pytest.mark.parametrize("what", ["all rays miss", "empty grid"])
def test_nothing_to_render(what):
    from apnrf_amd import render as RD
    c = _case()
    hip, est = H.hip_field(c["sc"]).train(), H.hip_estimator(c["sc"])
    rays = _rays(c)
    if what == "all rays miss":
        rays = RD.Rays(rays.origins[-N_MISS:].repeat(7, 1), rays.viewdirs[-N_MISS:].repeat(7, 1))      # 77 rays
    else:
        est.binaries = torch.zeros_like(est.binaries)
        est.occs = torch.zeros_like(est.occs)
    R_ = rays.origins.shape[0]
    rgb, acc, depth, sem, n = RD.fused_train_render(hip, est, rays, render_bkgd=BK.to(DEV), stratified=False, **H.RENDER_KW)
    assert n == 0
    assert torch.equal(rgb.detach().cpu(), BK.expand(R_, 3))
    assert float(acc.abs().max()) == 0.0 and float(depth.abs().max()) == 0.0 and float(sem.abs().max()) == 0.0
    (rgb.sum() + acc.sum() + depth.sum() + sem.sum()).backward()
    for p in _params(hip):
        assert p.grad is not None and float(p.grad.abs().max()) == 0.0
    last = RD.latest_train_render(hip)
    assert int(last["skip"]) > 0 and int(last["counts"][3]) == 16


# ------------------------------------------------------------------ 8. non-finite loss
@pytest.mark.parametrize("deterministic", [False, True])
def test_nan_loss_raises_the_flag_and_leaves_the_parameters_alone(deterministic):
    """(deterministic=True: the fixed-point accumulation's fills, conversion and reduction run with zero samples behind the raised flag)"""
    from apnrf_amd import render as RD
    from apnrf_amd.optim import FusedAdam
    c = _case()
    hip = H.hip_field(c["sc"]).train()
    opt = FusedAdam(hip.parameters(), lr=1e-3, eps=1e-15).bind_field(hip)
    before = [p.detach().clone() for p in hip.parameters()]
    pix, dep, lab = (t.to(DEV) for t in (c["pix"], c["dep"], c["lab"]))
    rgb, acc, depth, sem, n = RD.fused_train_render(hip, c["est"], _rays(c), render_bkgd=BK.to(DEV), stratified=False, deterministic=deterministic,
                                                    **H.RENDER_KW)
    last = RD.latest_train_render(hip)
    assert n > 500 and int(last["skip"]) == 0
    (_loss(rgb, depth, sem, pix, dep, lab) * float("nan")).backward()
    assert int(last["counts"][3]) == 32 and int(last["skip"]) > 0
    for p in _params(hip):
        assert bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) == 0.0
    opt.step(skip=last["skip"], count_nonfinite=True)
    assert all(torch.equal(p.detach(), b) for p, b in zip(hip.parameters(), before))
    assert all(float(opt.state[p]["step"]) == 0 for p in hip.parameters() if p.numel() and p in opt.state)


# ------------------------------------------------------------------ 9. misuse
def test_second_backward_and_changed_parameters_raise():
    from apnrf_amd import _lib as L
    from apnrf_amd import render as RD
    from apnrf_amd.optim import FusedAdam
    c = _case()
    hip = H.hip_field(c["sc"]).train()
    kw = dict(render_bkgd=BK.to(DEV), stratified=False, **H.RENDER_KW)
    rgb = RD.fused_train_render(hip, c["est"], _rays(c), **kw)[0]
    loss = rgb.sum()
    loss.backward(retain_graph=True)
    with pytest.raises(L.MnfError, match="second backward"):
        loss.backward()
    opt = FusedAdam(hip.parameters(), lr=1e-3, eps=1e-15).bind_field(hip)
    rgb = RD.fused_train_render(hip, c["est"], _rays(c), **kw)[0]
    opt.step()                                       # (the gradients of the backward above)
    with pytest.raises(L.MnfError, match="parameters changed"):
        rgb.sum().backward()


def test_five_level_estimator_hands_over_to_the_drop_in():
    from apnrf_amd import render as RD
    from apnrf_amd.nerfacc import OccGridEstimator
    roi = np.array([-12.0, 0.5, -12.0, -10.0, 1.5, -10.0], np.float32)
    est = OccGridEstimator(torch.from_numpy(roi), resolution=[20, 10, 20], levels=5)
    occ = np.random.default_rng(2).random((5, 20, 10, 20)) < np.array([0.15, 0.10, 0.08, 0.06, 0.05])[:, None, None, None]
    est.binaries = torch.from_numpy(occ)
    est.occs = torch.from_numpy(occ.reshape(-1).astype(np.float32)) * 0.05
    est = est.to(DEV)
    sc = H.make_scene(log2_hashmap_size=15, seed=6)
    fs = dict(sc); fs["aabb"] = est.aabbs[-1].cpu().numpy().astype(np.float32)
    o, d = H.view_rays(sc, 3, h=7, w=9)
    rays = RD.Rays((o + torch.tensor([3.0, 0.0, 3.0])).to(DEV), d.to(DEV))
    hip = H.hip_field(fs)
    got = RD.fused_train_render(hip.train(), est, rays, render_bkgd=BK.to(DEV), stratified=False, **H.RENDER_KW)
    assert hip.training and RD.latest_train_render(hip) is None
    want = RD.render_image_with_occgrid_with_depth_guide(hip.eval(), est, rays, render_bkgd=BK.to(DEV), **H.RENDER_KW)
    assert got[4] == want[4] and got[4] > 100 and got[0].requires_grad
    assert all(torch.equal(g, w) for g, w in zip(got[:4], want[:4]))


# ------------------------------------------------------------------ 10. train_step(loss_fn=...)
def test_train_step_with_a_loss_fn_equals_the_default_step():
    from apnrf_amd import render as RD
    from apnrf_amd.optim import FusedAdam
    c = _case()
    rays = _rays(c)
    pix, dep, lab = (t.to(DEV) for t in (c["pix"], c["dep"], c["lab"]))
    outs = []
    for loss_fn in (_loss7, None):
        hip = H.hip_field(c["sc"])
        opt = FusedAdam(hip.parameters(), lr=1e-3, eps=1e-15).bind_field(hip)
        before = [p.detach().clone() for p in hip.parameters()]
        out = RD.train_step(hip, H.hip_estimator(c["sc"]), opt, rays, pix, dep, lab, BK.to(DEV), step=1, stratified=False, loss_fn=loss_fn, **H.RENDER_KW)
        assert not out["skipped"] and out["n_rendering_samples"] == c["ref"][4]
        assert all(not torch.equal(p.detach(), b) for p, b in zip(hip.parameters(), before) if p.numel())      # the optimizer stepped every vector
        outs.append((out, hip))
    np.testing.assert_allclose(float(outs[0][0]["loss"]), float(outs[1][0]["loss"]), rtol=2e-5)
    hip = outs[0][1].eval()
    rgb2 = RD.render_views(hip, c["est"], rays.origins, rays.viewdirs, c["n"], 1024, render_bkgd=BK, **H.RENDER_KW)["rgb"]
    assert bool(torch.isfinite(rgb2).all())
    with pytest.raises(ValueError):
        RD.train_step(hip, H.hip_estimator(c["sc"]), opt, rays, pix, dep, lab, BK.to(DEV), step=1, sync=False, loss_fn=_loss7, **H.RENDER_KW)
