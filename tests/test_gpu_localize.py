"""GPU tests of the pose refiner (csrc/localize.hip, apnrf_amd/localize.py): its three stages against tests/localize_ref.py, a whole iteration against the
torch route it replaces (`transform_rays` -> `fused_train_render_rays` -> loss -> autograd), batch independence, and recovery of perturbed poses against
INTEGRATION.md §A's second loop.  Scene: `make_scene(log2_hashmap_size=15)`, shapes (128, 2, 29) and (64, 4, 13); images of 48 x 40 pixels.

Bars (each figure is printed before it is asserted):
  rays        2^-22 relative to the ray's norm against the restatement; R within 1 fp32 ulp (device and host sin / cos may differ in the last place of a
              double, and R is rounded once); targets and drawn pixel ids exact; with xi = 0 the bytes of `mnf_generate_rays` and `mnf_gather_pixels`
  loss        n 2^-24 sum|terms|: fp32 rounding of an n-term mean, the terms being what a value is formed from (for the cross-entropy log(den) and the
              shifted logit, for a gradient element the operands of its difference)
  update      2^-22 sum|terms| on the 6-vector gradient (the inputs are fp32-rounded), identical bytes on a second run, xi after Adam to 1e-12
  iteration   the project's bars for this backward (test_gpu_fused_ray_grads.py): rel L2 < 3e-2, cosine > 0.999; the rendered planes bit for bit
  recovery    per view, the refiner's last loss against the reference loop's plus the loop's own largest change over its last three iterations, and below
              the refiner's first; the scene (random parameters, else the trained small room) is chosen by the reference loop alone"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import helpers as H
import localize_ref as LR
from apnrf_amd import _lib as L

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(128, 2, 29), (64, 4, 13)]
HI, WI, N_IMAGES = 40, 48, 4
WEIGHTS = (10.0, 0.2, 0.5)
XI3 = np.array([[0.0] * 6, [2e-4, -3e-4, 1e-4, 0.01, -0.02, 0.005], [0.3 * 2 / 3, -0.3 * 2 / 3, 0.3 / 3, 0.2 * 0.6, 0.0, -0.2 * 0.8]])      # zero, small (series), 0.3 rad with 0.2 m
MAX_EMPTY_SHARE = 0.9      # no test leaves more than this share of its rays without kept samples


@functools.lru_cache(maxsize=None)
def _model(shape):
    sc = H.make_scene(neurons=shape[0], layers=shape[1], C=shape[2], log2_hashmap_size=15)
    field = H.hip_field(sc).train()
    field.requires_grad_(False)
    return sc, field, H.hip_estimator(sc)


def _c2w(sc, ids):
    from apnrf_amd import render as RD
    return np.stack([RD.pose_to_c2w(np.asarray(sc["poses"][i], np.float64)) for i in ids]).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _random_dataset(shape, packed):
    """N_IMAGES random u8 images with depths and labels inside [0, C), in the reference layout or the packed one"""
    import tempfile
    from apnrf_amd.dataset import Dataset
    sc = _model(shape)[0]
    rng = np.random.default_rng(5)
    ds = Dataset(training=False, save_fp=tempfile.mkdtemp(), device=DEV, packed=packed)
    ds.update_data(rng.integers(0, 256, (N_IMAGES, HI, WI, 3), dtype=np.uint8), rng.uniform(0.2, 6.0, (N_IMAGES, HI, WI)).astype(np.float32),
                   rng.integers(0, shape[2], (N_IMAGES, HI, WI)).astype(np.int64), _c2w(sc, [4, 1, 2, 6]))
    return ds


def _pose_opts(lr_rot=1e-3, lr_trans=2e-3, weights=WEIGHTS, seed=0):
    p = L.PoseOpts()
    p.w_rgb, p.w_dep, p.w_sem = weights
    p.lr_rot, p.lr_trans, p.beta1, p.beta2, p.eps, p.seed = lr_rot, lr_trans, 0.9, 0.999, 1e-15, seed
    return p


def _refiner(shape, image_ids, ds=None, **kw):
    from apnrf_amd.localize import PoseRefiner
    _, field, est = _model(shape)
    return PoseRefiner(field, est, ds if ds is not None else _random_dataset(shape, False), image_ids, **kw, **H.RENDER_KW)


def _kept(ref):
    """the kept-sample count of every ray of the refiner's latest iteration"""
    from apnrf_amd import localize as LZ
    return ref.last_iteration(LZ.WS_KEPT).cpu().numpy().copy()


def _check_sample_set(kept, name):
    """What the batches are chosen for, over the iterations of a test (`kept`: `_kept` of one iteration or a list of them): at least one ray keeps nothing, the
    longest ray crosses a 64-sample tile, and most rays keep something"""
    kept = np.concatenate([np.asarray(k).reshape(-1) for k in (kept if isinstance(kept, list) else [kept])])
    empty = float((kept == 0).mean())
    print(f"{name}: kept samples per ray {kept[kept > 0].min() if (kept > 0).any() else 0} .. {kept.max()}, {int((kept == 0).sum())} of {kept.size} rays keep none "
          f"(share {empty:.3f}, bar {MAX_EMPTY_SHARE})")
    assert (kept == 0).sum() >= 1, "at least one ray keeps nothing"
    assert kept.max() > 64, "the longest ray must cross a 64-sample tile"
    assert empty <= MAX_EMPTY_SHARE


# ------------------------------------------------------------------ rays and targets
@pytest.mark.parametrize("packed", [False, True], ids=["reference-layout", "packed"])
def test_rays_and_targets(packed):
    shape = SHAPES[0]
    ds = _random_dataset(shape, packed)
    assert ds.depths.dtype == (torch.float16 if packed else torch.float32) and ds.semantics.dtype == (torch.uint8 if packed else torch.int64)
    ids, n = [2, 0, 3], 193
    ref = _refiner(shape, ids, ds, rays_per_view=n, seed=77)
    ref.xi.copy_(torch.from_numpy(XI3))
    got = {k: v.cpu().numpy() for k, v in ref.formed(0).items()}
    nxt = ref.formed(1)["pix"].cpu().numpy()
    # drawn pixel ids: exact, in range, new every iteration
    assert np.array_equal(got["pix"], LR.draw_pixels(3, n, 0, 77, WI, HI)) and np.array_equal(nxt, LR.draw_pixels(3, n, 1, 77, WI, HI))
    assert got["pix"].min() >= 0 and got["pix"].max() < WI * HI and (got["pix"] != nxt).mean() > 0.9
    c2w0 = ds.camtoworlds[torch.tensor(ids, device=DEV)][:, :3, :4].cpu().numpy()
    o, d, R = LR.pose_rays(c2w0, ds._focal, WI, HI, got["pix"], XI3)
    ulp = np.spacing(np.abs(R).astype(np.float32))
    r_err = float((np.abs(got["R"] - R) / ulp).max())
    d_err = float((np.linalg.norm(got["viewdirs"].astype(np.float64) - d, axis=-1) / np.linalg.norm(d.astype(np.float64), axis=-1)).max())
    o_err = float((np.linalg.norm(got["origins"].astype(np.float64) - o, axis=-1) / np.linalg.norm(o.astype(np.float64), axis=-1)).max())
    print(f"R: worst entry {r_err:.2f} ulp (bar 1); directions {d_err:.3e}, origins {o_err:.3e} relative to the ray's norm (bar {2.0 ** -22:.3e})")
    assert r_err <= 1.0 and d_err <= 2.0 ** -22 and o_err <= 2.0 ** -22
    assert np.array_equal(got["R"][0], np.eye(3, dtype=np.float32)) and np.array_equal(got["viewdirs"][0], d[0])      # xi = 0 changes no bit
    t_rgb, t_dep, t_lab = LR.targets(ds.images.cpu().numpy(), ds.depths.cpu().numpy(), ds.semantics.cpu().numpy(), ids, got["pix"])
    assert got["rgb"].tobytes() == t_rgb.tobytes() and got["dep"].tobytes() == t_dep.tobytes() and got["sem"].tobytes() == t_lab.tobytes()
    # the caller's pixels are used as given
    pix = torch.from_numpy(np.random.default_rng(0).integers(0, WI * HI, (3, n))).to(DEV)
    fixed = _refiner(shape, ids, ds, rays_per_view=n, pix_idx=pix)
    assert torch.equal(fixed.formed(0)["pix"], pix) and torch.equal(fixed.formed(5)["pix"], pix)


@pytest.mark.parametrize("packed", [False, True], ids=["reference-layout", "packed"])
def test_pose_rays_equal_raygen_and_gather(packed):
    """With xi = 0, `mnf_pose_rays` gives the bytes of `mnf_generate_rays` and `mnf_gather_pixels`, called per view with the same pixels: 7 x 5 images (both
    centres are half-integers), 3 of them, views of images [2, 0], 70 caller's pixels per view (more than a wave, no multiple of 64; pixels 0 and 34 among
    them), float32 poses with a general rotation (no direction component is zero)."""
    from apnrf_amd.localize import rodrigues
    W, Hh, n_img, B, n, C = 7, 5, 3, 2, 70, 11
    rng = np.random.default_rng(12)
    images = torch.from_numpy(rng.integers(0, 256, (n_img, Hh, W, 3), dtype=np.uint8)).to(DEV)
    depths = torch.from_numpy(rng.uniform(0.2, 6.0, (n_img, Hh, W)).astype(np.float16 if packed else np.float32)).to(DEV)
    sems = torch.from_numpy(rng.integers(0, C, (n_img, Hh, W)).astype(np.uint8 if packed else np.int64)).to(DEV)
    ids = torch.tensor([2, 0], dtype=torch.int64, device=DEV)
    pix_np = rng.integers(0, W * Hh, (B, n))
    pix_np[0, 0], pix_np[0, 69], pix_np[1, 64], pix_np[1, 3] = 0, W * Hh - 1, 0, W * Hh - 1
    pix = torch.from_numpy(pix_np).to(DEV)
    c2w_np = np.zeros((B, 3, 4))
    c2w_np[0, :, :3], c2w_np[1, :, :3] = rodrigues(np.array([0.4, -0.7, 0.55])), rodrigues(np.array([-1.1, 0.3, 0.8]))
    c2w_np[:, :, 3] = [[0.3, 1.1, -0.7], [-1.4, 0.9, 2.2]]
    c2w = torch.from_numpy(c2w_np.astype(np.float32)).to(DEV)
    focal = float(np.float32(4.3))
    xi = torch.zeros(B, 6, dtype=torch.float64, device=DEV)
    lib = L.load_library()
    o, d = torch.empty(B, n, 3, device=DEV), torch.empty(B, n, 3, device=DEV)
    pix_out, rot = torch.empty(B, n, dtype=torch.int64, device=DEV), torch.empty(B, 3, 3, device=DEV)
    rgb, dep, lab = torch.empty(B, n, 3, device=DEV), torch.empty(B, n, device=DEV), torch.empty(B, n, dtype=torch.int64, device=DEV)
    L.launch(lib.mnf_pose_rays, L.ptr(images), L.ptr(depths), int(packed), L.ptr(sems), int(packed), n_img, L.ptr(ids), L.ptr(c2w), focal, W, Hh, L.ptr(pix), L.ptr(xi),
             B, n, 0, 0, L.ptr(o), L.ptr(d), L.ptr(pix_out), L.ptr(rot), L.ptr(rgb), L.ptr(dep), L.ptr(lab))
    assert torch.equal(pix_out, pix)
    for b in range(B):
        o1, d1 = torch.empty(1, n, 3, device=DEV), torch.empty(1, n, 3, device=DEV)
        rgb1, dep1, lab1 = torch.empty(n, 3, device=DEV), torch.empty(n, device=DEV), torch.empty(n, dtype=torch.int64, device=DEV)
        view_pix = pix[b].contiguous()
        L.launch(lib.mnf_generate_rays, L.ptr(c2w[b:b + 1].contiguous()), 1, W, Hh, focal, L.ptr(view_pix), n, L.ptr(o1), L.ptr(d1))
        L.launch(lib.mnf_gather_pixels, L.ptr(images), L.ptr(depths), int(packed), L.ptr(sems), int(packed), W * Hh, L.ptr(ids[b:b + 1].contiguous()), L.ptr(view_pix),
                 n, L.ptr(rgb1), L.ptr(dep1), L.ptr(lab1))
        assert (d1 != 0).all(), "a general rotation: no direction component is zero"
        for name, got, want in (("origins", o[b], o1[0]), ("directions", d[b], d1[0]), ("rgb", rgb[b], rgb1), ("depth", dep[b], dep1), ("labels", lab[b], lab1)):
            assert got.cpu().numpy().tobytes() == want.cpu().numpy().tobytes(), f"view {b}: {name} differ"


# ------------------------------------------------------------------ loss
@pytest.mark.parametrize("n", [193, 1500])
def test_loss_against_torch(n):
    B, C = 3, 13
    rng = np.random.default_rng(n)
    rgb, depth, sem = rng.random((B, n, 3), np.float32), rng.uniform(0, 6, (B, n)).astype(np.float32), (rng.standard_normal((B, n, C)) * 3).astype(np.float32)
    t_rgb, t_dep = rng.random((B, n, 3), np.float32), rng.uniform(0, 6, (B, n)).astype(np.float32)
    t_lab = rng.integers(0, C, (B, n)).astype(np.int64)
    t_lab[1, n // 2] = C      # one view carries a bad label
    want = LR.pose_loss(rgb, depth, sem, t_rgb, t_dep, t_lab, WEIGHTS)
    dev = [torch.from_numpy(x).to(DEV) for x in (rgb, depth, sem, t_rgb, t_dep, t_lab)]
    loss, status, word = torch.zeros(B, dtype=torch.float64, device=DEV), torch.full((B,), -1, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int64, device=DEV)
    g = [torch.full_like(dev[0], 7.0), torch.full_like(dev[1], 7.0), torch.full_like(dev[2], 7.0)]
    pose = _pose_opts()
    L.launch(L.load_library().mnf_pose_loss, *(L.ptr(x) for x in dev), B, n, C, ctypes.byref(pose), L.ptr(loss), *(L.ptr(x) for x in g), L.ptr(status), L.ptr(word))
    assert status.tolist() == [0, 8, 0] == want[4].tolist() and int(word) == 8
    # sum|terms| of a view's loss: what its three means are formed from
    lse = np.log(np.exp(sem.astype(np.float64) - sem.max(-1, keepdims=True)).sum(-1))
    lab_ok = np.clip(t_lab, 0, C - 1)
    shifted = np.abs(np.take_along_axis(sem, lab_ok[..., None], -1)[..., 0].astype(np.float64) - sem.max(-1))
    sl1 = lambda x: np.where(np.abs(x) < 1, 0.5 * x * x, np.abs(x) - 0.5)
    terms = (WEIGHTS[0] / 3 * sl1(rgb.astype(np.float64) - t_rgb).sum((1, 2)) + WEIGHTS[1] * sl1(depth.astype(np.float64) - t_dep).sum(1)
             + WEIGHTS[2] * (np.abs(lse) + shifted).sum(1)) / n
    bar = n * 2.0 ** -24 * terms
    err = np.abs(loss.cpu().numpy() - want[0])
    print(f"n = {n}: per-view loss {want[0]}, abs err {err} (bar {bar})")
    assert (err <= bar).all()
    p = np.exp(sem.astype(np.float64) - sem.max(-1, keepdims=True))
    p /= p.sum(-1, keepdims=True)
    onehot = (np.arange(C)[None, None] == t_lab[..., None]).astype(np.float64)
    g_terms = [WEIGHTS[0] / 3 / n * (np.abs(rgb) + np.abs(t_rgb)), WEIGHTS[1] / n * (np.abs(depth) + np.abs(t_dep)), WEIGHTS[2] / n * (p + onehot)]
    for name, got, ref, tm in zip(("g_rgb", "g_depth", "g_sem"), g, want[1:4], g_terms):
        got = got.cpu().numpy().astype(np.float64)
        assert (got[1] == 0).all(), f"{name}: the flagged view's gradients are zero"
        ratio = float((np.abs(got - ref)[[0, 2]] / (n * 2.0 ** -24 * tm[[0, 2]])).max())
        print(f"n = {n}: {name} worst error / bar {ratio:.3e}")
        assert ratio <= 1.0


# ------------------------------------------------------------------ update
def _update_inputs(n, seed):
    rng = np.random.default_rng(seed)
    B = 4
    g_o, g_d = (rng.standard_normal((B, n, 3)) * 1e-3).astype(np.float32), (rng.standard_normal((B, n, 3)) * 1e-3).astype(np.float32)
    d = rng.standard_normal((B, n, 3))
    d = (d / np.linalg.norm(d, axis=-1, keepdims=True)).astype(np.float32)
    xi = np.concatenate([XI3, [[1.5, -1.2, 1.6, 0.3, 0.1, -0.2]]])      # |rotvec| = 2.5 for the fourth view
    m, v = rng.standard_normal((B, 6)) * 1e-3, rng.random((B, 6)) * 1e-6
    return g_o, g_d, d, xi, m, v


def _run_update(g_o, g_d, d, xi, m, v, stalled, iteration, pose, kept=None, status=None, skip=None):
    t = lambda a, dt: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(DEV)
    B, n = g_o.shape[:2]
    dev = dict(g_o=t(g_o, torch.float32), g_d=t(g_d, torch.float32), d=t(d, torch.float32), kept=t(kept, torch.int64), status=t(status, torch.int32),
               skip=t(skip, torch.int32), xi=t(xi, torch.float64), m=t(m, torch.float64), v=t(v, torch.float64), stalled=t(stalled, torch.int32))
    grad = torch.zeros(B, 6, dtype=torch.float64, device=DEV)
    L.launch(L.load_library().mnf_pose_update, L.ptr(dev["g_o"]), L.ptr(dev["g_d"]), L.ptr(dev["d"]), L.ptr(dev["kept"]), L.ptr(dev["status"]), L.ptr(dev["skip"]), B, n,
             iteration, ctypes.byref(pose), L.ptr(dev["xi"]), L.ptr(dev["m"]), L.ptr(dev["v"]), L.ptr(dev["stalled"]), L.ptr(grad))
    return tuple(dev[k].cpu().numpy() for k in ("xi", "m", "v", "stalled")) + (grad.cpu().numpy(),)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
def test_update_gradient_and_adam(n):
    g_o, g_d, d, xi, m, v = _update_inputs(n, n)
    pose, stalled, iteration = _pose_opts(lr_rot=2e-3, lr_trans=7e-3), np.array([0, 1, 0, 2]), 4
    got = _run_update(g_o, g_d, d, xi, m, v, stalled, iteration, pose)
    again = _run_update(g_o, g_d, d, xi, m, v, stalled, iteration, pose)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again)), "two runs give identical bytes"
    want = LR.pose_update(g_o, g_d, d, None, None, 0, xi, m, v, stalled, iteration, 2e-3, 7e-3)
    for b in range(4):
        ref, terms = LR.pose_gradient(g_o[b], g_d[b], d[b], xi[b, :3])
        bar = 2.0 ** -22 * np.concatenate([np.full(3, terms[:3].sum()), terms[3:]])      # (J_l^T mixes the three sums of the rotation part)
        err = np.abs(got[4][b] - ref)
        print(f"n = {n}, view {b}: gradient abs err {err.max():.3e} (smallest bar {bar.min():.3e})")
        assert (err <= bar).all()
    assert np.array_equal(got[3], stalled) and np.abs(got[0] - want[0]).max() < 1e-12 and (got[0] != xi).all()
    print(f"n = {n}: xi after the Adam step differs from the restatement by {np.abs(got[0] - want[0]).max():.3e} (bar 1e-12)")
    assert np.abs(got[1] - want[1]).max() < 1e-15 and np.abs(got[2] - want[2]).max() < 1e-18


def test_update_skip_rules():
    n = 65
    g_o, g_d, d, xi, m, v = _update_inputs(n, 3)
    pose, stalled = _pose_opts(), np.array([0, 0, 5, 0])
    kept = np.ones((4, n), np.int64)
    kept[1] = 0                                       # view 1 kept no sample
    status = np.array([0, 0, 8, 0], np.int32)         # view 2 carries its status bit
    got = _run_update(g_o, g_d, d, xi, m, v, stalled, 0, pose, kept, status, np.zeros(1))
    assert got[3].tolist() == [0, 1, 6, 0]
    for b in (1, 2):
        assert got[0][b].tobytes() == xi[b].tobytes() and got[1][b].tobytes() == m[b].tobytes() and got[2][b].tobytes() == v[b].tobytes()
    assert (got[0][[0, 3]] != xi[[0, 3]]).all()
    got = _run_update(g_o, g_d, d, xi, m, v, stalled, 0, pose, kept, status, np.ones(1))      # the render's skip flag: every view is left alone
    assert got[3].tolist() == [1, 1, 6, 1] and got[0].tobytes() == xi.tobytes() and got[1].tobytes() == m.tobytes() and got[2].tobytes() == v.tobytes()
    g_bad = g_d.copy()
    g_bad[3, 7, 1] = np.nan                           # a gradient that is not finite stalls its view only
    got = _run_update(g_o, g_bad, d, xi, m, v, stalled, 0, pose, kept, status, np.zeros(1))
    assert got[3].tolist() == [0, 1, 6, 1] and got[0][3].tobytes() == xi[3].tobytes()


# ------------------------------------------------------------------ a whole iteration against the torch route
def _view_losses(planes, tg, B, n):
    """the refiner's loss in torch: per view, each mean over the view's own rays -> [B]"""
    import torch.nn.functional as F
    rgb, depth, sem = planes[0].view(B, n, 3), planes[2].view(B, n), planes[3].view(B, n, -1)
    return torch.stack([WEIGHTS[0] * F.smooth_l1_loss(rgb[b], tg["rgb"][b]) + WEIGHTS[1] * F.smooth_l1_loss(depth[b], tg["dep"][b])
                        + WEIGHTS[2] * F.cross_entropy(sem[b], tg["sem"][b]) for b in range(B)])


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_whole_iteration_teacher_forced(shape):
    from apnrf_amd import localize as LZ
    from apnrf_amd import render as RD
    from test_gpu_input_grads import _figures
    _, field, est = _model(shape)
    ids, n, B = [0, 2], 193, 2
    ref = _refiner(shape, ids, rays_per_view=n, seed=9, lr_rot=1e-3, lr_trans=2e-3)
    base = _refiner(shape, ids, rays_per_view=n, seed=9)      # xi stays 0: the un-corrected rays of every iteration
    ref.xi.copy_(torch.tensor([[0.01, -0.02, 0.015, 0.02, -0.01, 0.015], [-0.008, 0.004, 0.01, -0.03, 0.02, 0.01]], dtype=torch.float64))
    kept = []
    for it in range(3):
        xi_now = ref.xi.cpu().numpy().copy()
        formed, plain = ref.formed(), base.formed(it)
        assert torch.equal(formed["pix"], plain["pix"])
        ref.step(1)
        assert torch.equal(ref.last_iteration(LZ.WS_RAYS_O), formed["origins"]) and torch.equal(ref.last_iteration(LZ.WS_RAYS_D), formed["viewdirs"])
        got_planes = [ref.last_iteration(w).clone() for w in (LZ.WS_RGB, LZ.WS_ACC, LZ.WS_DEPTH, LZ.WS_SEM)]
        got_grad = ref.last_iteration(LZ.WS_GRAD).cpu().numpy().copy()
        kept.append(_kept(ref))
        o, d = formed["origins"].clone().requires_grad_(), formed["viewdirs"].clone().requires_grad_()
        planes = RD.fused_train_render_rays(field, est, RD.Rays(o.view(-1, 3), d.view(-1, 3)), stratified=False, **H.RENDER_KW)[:4]
        for name, a, b in zip(("rgb", "acc", "depth", "sem"), got_planes, planes):
            same = torch.equal(a.reshape(-1), b.detach().reshape(-1))
            print(f"iteration {it}: plane {name} bit-identical on both routes: {same}" + ("" if same else f" (max abs diff {float((a.reshape(-1) - b.detach().reshape(-1)).abs().max()):.3e})"))
            assert same
        losses = _view_losses(planes, formed, B, n)
        losses.sum().backward()
        trace = ref.result()
        assert np.abs(trace["loss_trace"][it] - losses.detach().cpu().numpy()).max() < 1e-4 * float(losses.max())
        assert trace["stalled"].tolist() == [0, 0] and trace["status"] == 0
        for b in range(B):
            rot, tr = torch.tensor(xi_now[b, :3], requires_grad=True), torch.tensor(xi_now[b, 3:], requires_grad=True)
            moved = RD.transform_rays(RD.Rays(plain["origins"][b].double().cpu(), plain["viewdirs"][b].double().cpu()), rot, tr)
            ((o.grad[b].double().cpu() * moved.origins).sum() + (d.grad[b].double().cpu() * moved.viewdirs).sum()).backward()
            want = np.concatenate([rot.grad.numpy(), tr.grad.numpy()])
            err, c = _figures(torch.from_numpy(got_grad[b]), torch.from_numpy(want))
            print(f"iteration {it}, view {b}: 6-vector gradient rel L2 err {err:.3e}, cos {c:.6f}  (bar 3e-2, 0.999)")
            assert err < 3e-2 and c > 0.999
    _check_sample_set(kept, "three iterations")


def test_batch_independence():
    """Views {a, b, c} together and view b alone, with the same pixels, seed and iterations: view b's xi has identical bytes (the forward's alpha threshold is
    the mean of the occupancy grid, no function of the batch)."""
    shape, n = SHAPES[0], 193
    pix = torch.from_numpy(np.random.default_rng(4).integers(0, WI * HI, (3, n))).to(DEV)
    x0 = torch.tensor([0.004, -0.006, 0.005, 0.02, -0.01, 0.015], dtype=torch.float64)
    three, one = _refiner(shape, [0, 2, 3], rays_per_view=n, pix_idx=pix), _refiner(shape, [2], rays_per_view=n, pix_idx=pix[1:2])
    three.xi[1].copy_(x0)
    one.xi[0].copy_(x0)
    three.step(3)
    one.step(3)
    _check_sample_set(_kept(three), "three views")
    a, b = three.result(), one.result()
    print(f"view b refined alone {b['xi'][0]}, among three {a['xi'][1]}")
    assert a["stalled"].tolist() == [0, 0, 0] and b["stalled"].tolist() == [0] and a["status"] == 0 and b["status"] == 0
    assert (a["xi"][1] != x0.numpy()).all()
    assert a["xi"][1].tobytes() == b["xi"][0].tobytes() and a["loss_trace"][:, 1].tobytes() == b["loss_trace"][:, 0].tobytes()


def test_bad_label_stalls_its_view_only():
    shape, n = SHAPES[1], 193
    ds = _random_dataset(shape, False)
    sem = ds.semantics.clone()
    try:
        ds.semantics[1] = shape[2]      # every label of image 1 lies outside the classes
        ref = _refiner(shape, [0, 1], ds, rays_per_view=n)
        ref.step(2)
        out = ref.result()
    finally:
        ds.semantics.copy_(sem)
    assert out["stalled"].tolist() == [0, 2] and out["status"] & 8 and (out["xi"][1] == 0).all() and (out["xi"][0] != 0).all()


# ------------------------------------------------------------------ recovery against the reference loop
def _rendered_dataset(field, est, c2w, side_h, side_w, kw):
    """The field's own renders at the poses `c2w`, stored through Dataset.update_data: u8 colours, fp32 depths, argmax labels"""
    import tempfile
    from apnrf_amd import render as RD
    from apnrf_amd.dataset import Dataset
    ds = Dataset(training=False, save_fp=tempfile.mkdtemp(), device=DEV)
    focal = 0.5 * side_w / np.tan(np.pi / 4)
    K = torch.tensor([[focal, 0, side_w / 2], [0, focal, side_h / 2], [0, 0, 1]])
    rays = RD.generate_image_rays(c2w, side_w, side_h, K, DEV)
    with torch.no_grad():
        rgb, _, depth, sem, _ = RD.fused_train_render_rays(field, est, RD.Rays(rays.origins.reshape(-1, 3), rays.viewdirs.reshape(-1, 3)), stratified=False, **kw)
    V = c2w.shape[0]
    ds.update_data((rgb.view(V, side_h, side_w, 3).clamp(0, 1) * 255).round().to(torch.uint8), depth.view(V, side_h, side_w), sem.view(V, side_h, side_w, -1).argmax(-1),
                   torch.from_numpy(c2w))
    return ds


def _perturbed(c2w, deg, cm):
    """every pose rotated by `deg` about a fixed axis and moved by `cm` along a fixed direction"""
    from apnrf_amd.localize import rodrigues
    axis, direction = np.array([0.36, 0.8, -0.48]), np.array([0.6, 0.0, 0.8])
    out = c2w.astype(np.float64).copy()
    out[:, :3, :3] = rodrigues(axis * np.deg2rad(deg)) @ out[:, :3, :3]
    out[:, :3, 3] += direction * cm * 1e-2
    return out.astype(np.float32)


def _reference_loop(field, est, kw, base, b, iters, lr):
    """INTEGRATION.md §A's second loop as it stands there (one fp32 6-vector, `torch.optim.Adam([xi], lr=1e-3)`) on view b alone, with the refiner's pixels and
    loss -> (loss trace [iters], xi after every iteration)"""
    from apnrf_amd import render as RD
    xi = torch.zeros(6, device=DEV, requires_grad=True)
    opt = torch.optim.Adam([xi], lr=lr)
    trace, xis = [], []
    for it in range(iters):
        f = base.formed(it)
        rays = RD.transform_rays(RD.Rays(f["origins"][b], f["viewdirs"][b]), xi[:3], xi[3:])
        planes = RD.fused_train_render_rays(field, est, rays, stratified=False, **kw)[:4]
        loss = _view_losses(planes, {k: v[b:b + 1] for k, v in f.items()}, 1, f["pix"].shape[1])[0]
        opt.zero_grad()
        loss.backward()
        opt.step()
        trace.append(float(loss.detach()))
        xis.append(xi.detach().cpu().numpy().astype(np.float64))
    return np.array(trace), np.array(xis)


def _pose_error(c2w, truth):
    """per view: (rotation error in degrees, translation error in cm)"""
    c2w, truth = np.asarray(c2w, np.float64), np.asarray(truth, np.float64)
    rel = np.einsum("nij,nkj->nik", c2w[:, :3, :3], truth[:, :3, :3])
    return (np.degrees(np.arccos(np.clip((np.trace(rel, axis1=1, axis2=2) - 1.0) / 2.0, -1.0, 1.0))), 100.0 * np.linalg.norm(c2w[:, :3, 3] - truth[:, :3, 3], axis=1))


def _recover(field, est, kw, ds, c2w, n, name, iters=20, lr=1e-3):
    """The recovery run on one scene: the ladder on the reference loop alone, then the refiner from the same start, per view -> what the two did.
    Learning rate: the documented loop's own, 1e-3 for all six numbers, on both routes (the smallest rung, 8.7e-3 rad and 1 cm, is within reach of 20 such steps)."""
    lr_rot = lr_trans = lr
    from apnrf_amd.localize import PoseRefiner
    B = c2w.shape[0]
    mk = lambda start, **more: PoseRefiner(field, est, ds, list(range(B)), c2w0=start, rays_per_view=n, pix_idx=pix, **more, **kw)
    pix = torch.from_numpy(np.random.default_rng(8).integers(0, ds.width * ds.height, (B, n))).to(DEV)
    for deg, cm in ((0.5, 1.0), (1.0, 2.0), (2.0, 5.0)):
        start = _perturbed(c2w, deg, cm)
        base = mk(start)
        both = [_reference_loop(field, est, kw, base, b, iters, lr) for b in range(B)]
        loops, loop_xi = [t for t, _ in both], [x for _, x in both]
        for b, t in enumerate(loops):
            print(f"{name}: perturbation ({deg} deg, {cm} cm), reference loop, view {b}: " + " ".join(f"{x:.5f}" for x in t))
        if all(t[-1] < t[0] for t in loops):
            break
    else:
        print(f"{name}: the reference loop's loss falls for no perturbation of the ladder")
        return None
    # how rough the loss is as a function of the pose here: the 6-vector gradient at the start and 1e-6 m beside it (printed, no bar)
    probe = mk(start, lr_rot=0.0, lr_trans=0.0)
    probe.step(1)
    g0 = probe.last_iteration(9).cpu().numpy().copy()
    probe.xi[:, 3] += 1e-6
    probe.step(1)
    g1 = probe.last_iteration(9).cpu().numpy().copy()
    print(f"{name}: the 6-vector gradient moves by " + ", ".join(f"{np.linalg.norm(g1[b] - g0[b]) / np.linalg.norm(g0[b]):.3e}" for b in range(B))
          + " of its norm when the camera moves by 1e-6 m (per view)")
    ref = mk(start, lr_rot=lr_rot, lr_trans=lr_trans)
    xis, kept = [], []
    for _ in range(iters):
        ref.step(1)
        xis.append(ref.xi.clone())
    kept.append(_kept(ref))
    out = ref.result()
    xis = torch.stack(xis).cpu().numpy()
    assert out["stalled"].tolist() == [0] * B and out["status"] == 0
    for b in range(B):
        for it in (0, 1, 2, iters - 1):
            print(f"{name}: view {b}, xi after iteration {it}: refiner {np.array2string(xis[it, b], precision=6)}  loop {np.array2string(loop_xi[b][it], precision=6)}")
    e0, e1 = _pose_error(start, c2w), _pose_error(out["c2w"], c2w)
    print(f"{name}: pose error per view {e0[0]} deg, {e0[1]} cm at the start -> {e1[0]} deg, {e1[1]} cm refined")
    for b in range(B):
        print(f"{name}: view {b}: refiner " + " ".join(f"{x:.5f}" for x in out["loss_trace"][:, b]))
    return dict(out=out, kept=kept, loops=loops, start_error=e0, end_error=e1)


def _issue_bars(r, name):
    """Per view: the refiner's last loss does not exceed the reference loop's by more than the loop's own largest change between consecutive iterations over its
    last three, and lies below the refiner's own first loss"""
    failures = []
    for b, theirs in enumerate(r["loops"]):
        mine = r["out"]["loss_trace"][:, b]
        slack = float(np.abs(np.diff(theirs[-3:])).max())
        print(f"{name}: view {b}: refiner's last {mine[-1]:.5f} against the loop's {theirs[-1]:.5f} + {slack:.5f}; refiner's first {mine[0]:.5f}")
        if not (mine[-1] <= theirs[-1] + slack and mine[-1] < mine[0]):
            failures.append(b)
    assert not failures, f"{name}: views {failures} end above the reference loop's last loss plus its own late change, or not below their first loss"


def _trained_room():
    """tools/active_loop.py's small room: a closed procedural world seen by the scene sensor, a 128 x 2 field with a 2^14 table trained for 300 `train_step`s on
    the 12 captures of the initial yaw sweep -> (field, estimator, render options, the sweep's poses as c2w)"""
    from apnrf_amd import nerfacc as NA
    from apnrf_amd import render as RD
    from apnrf_amd import sensor as SN
    from apnrf_amd import synthetic as S
    from apnrf_amd.dataset import Dataset
    from apnrf_amd.ngp import NGPRadianceField
    from apnrf_amd.optim import FusedAdam
    aabb, cell, side, start, seed = np.array([-4.0, -0.2, -4.0, 4.0, 2.2, 4.0]), 0.2, 64, np.array([-2.0, 1.0, -2.0]), 3
    kw = dict(near_plane=0.1, render_step_size=5e-3, cone_angle=0.004, alpha_thre=0.01)
    torch.manual_seed(seed)
    res = [int(round((aabb[3 + k] - aabb[k]) / cell)) for k in range(3)]
    occ = S.make_occupancy(res, seed=seed, clutter=0.01, aabb=aabb, free_at=[start])
    sim = SN.VoxelSim(SN.VoxelScene.from_occupancy(occ, aabb, cell=cell, refine=2, closed=True, device=DEV), side, side)
    aabb32 = torch.from_numpy(aabb.astype(np.float32))
    field = NGPRadianceField(aabb=aabb32, neurons=128, layers=2, num_semantic_classes=29, log2_hashmap_size=14, seed=seed).to(DEV)
    est = NA.OccGridEstimator(aabb32, resolution=res, levels=1).to(DEV)
    opt = FusedAdam(field.parameters(), lr=2e-3, eps=1e-15).bind_field(field)
    data = Dataset(training=True, save_fp="", num_rays=1024, device=DEV)
    poses = S.camera_poses(start, 12)
    c2w = np.stack([RD.pose_to_c2w(np.asarray(p, np.float64)) for p in poses]).astype(np.float32)
    rgba, depth_ray, sem = sim.sample_images_from_poses(poses, depth="ray")
    data.update_data(rgba[..., :3], depth_ray, sem, torch.from_numpy(c2w).to(DEV))
    for step in range(300):
        b = data[0]
        RD.train_step(field, est, opt, b["rays"], b["pixels"], b["dep"], b["sem"], b["color_bkgd"], step=step, occ_thre=1e-2, deterministic=True, **kw)
    field.requires_grad_(False)
    return field, est, kw, c2w, side



def test_recovery_against_the_reference_loop():
    """Targets: the field's own renders at the true poses, stored through `Dataset.update_data`; start: every pose rotated and moved by the ladder's rung; 512
    fixed pixels per view; the reference: INTEGRATION.md §A's second loop as it stands there (`torch.optim.Adam([xi], lr=1e-3)`), one view at a time; the refiner
    with the same learning rate for all six numbers; 20 iterations.  Bars: `_issue_bars`.

    The scene is chosen by the reference loop alone.  On the random-parameter scene (poses 4 and 1, 48 x 40 renders) its loss must fall from first to last
    iteration for every view at some rung; measured on an MI355X it does not: view 0 falls at the first rung (1.62718 -> 1.61775) but view 1 rises at every rung
    (1.63140 -> 1.66035, 1.65578 -> 1.66090, 1.68776 -> 1.69028) — half the loss is the cross-entropy of a nearly uniform 29-class distribution, and the kept
    samples of a random field carry gradients of independent sign.  So the scene is the one named for that case: the small room of tools/active_loop.py, the
    field trained for 300 `train_step`s on the sensor's sweep, two of the sweep's poses, 64 x 64 renders.  There the loop falls at the first rung (0.35611 ->
    0.19365, 0.81813 -> 0.32863) and the refiner ends at 0.19341 (bar 0.19365 + 0.00239) and 0.32460 (bar 0.32863 + 0.01000); the pose errors go from 0.50 deg /
    1.00 cm to 0.11 deg / 0.31 cm and 0.04 deg / 0.35 cm.  The two routes take the same first step and agree to 1e-6 after the second; later they drift apart
    (the rays differ in their fp32 rounding, and with a constant sample set the 6-vector gradient moves by 1.4e-3 of its norm per micrometre of camera motion:
    `_recover` prints it), which is what the bar's slack is for.  On that scene the test also holds the refined poses to be closer to the truth than the start."""
    shape, n = SHAPES[0], 512
    sc, field, est = _model(shape)
    c2w = _c2w(sc, [4, 1])
    ds = _rendered_dataset(field, est, c2w, HI, WI, H.RENDER_KW)
    name = "random scene"
    r = _recover(field, est, H.RENDER_KW, ds, c2w, n, name)
    if r is None:
        name = "trained room"
        field, est, kw, c2w, side = _trained_room()
        c2w = c2w[[0, 5]]
        ds = _rendered_dataset(field, est, c2w, side, side, kw)
        r = _recover(field, est, kw, ds, c2w, n, name)
        assert r is not None, "the reference loop's loss falls for no perturbation of the ladder on either scene"
        assert (r["end_error"][0] < r["start_error"][0]).all() and (r["end_error"][1] < r["start_error"][1]).all()
    kept = np.concatenate([k.reshape(-1) for k in r["kept"]])
    print(f"{name}: kept samples per ray {kept.min()} .. {kept.max()}, {int((kept == 0).sum())} of {kept.size} rays keep none (share bar {MAX_EMPTY_SHARE})")
    assert (kept == 0).mean() <= MAX_EMPTY_SHARE and kept.max() > 64
    _issue_bars(r, name)
    # the refined poses go back into the dataset, from a device tensor or a host array, whatever the stored shape
    out = r["out"]
    ds.set_camtoworlds(torch.tensor([1], device=DEV), torch.from_numpy(out["c2w"][1:]).to(DEV))
    ds.set_camtoworlds([0], out["c2w"][:1, :3])
    assert torch.equal(ds.camtoworlds.cpu()[:, :3], torch.from_numpy(out["c2w"]).to(torch.float32)[:, :3])
    with pytest.raises(ValueError):
        ds.set_camtoworlds([0, 1], out["c2w"][:1])
