"""The restatement of the pose refiner (tests/localize_ref.py) against what the repository already trusts, and the unit's place in the header, the binding
table and the built library.  No GPU.

  pose gradient   dL/d(rotvec, trans) = (J_l^T sum d' x g_d, sum g_o) against float64 torch autograd through `render.transform_rays` of
                  sum(g_o . o' + g_d . d') for random g_o, g_d, at rotvec = 0, t^2 just below and just above the series threshold 1e-6, |rotvec| = 0.3
                  and 2.5.  Relative bar 1e-9 (float64 against float64; the series' truncation at the threshold is ~t^6/362880 ~ 3e-15).
  Adam            20 steps of a recorded gradient sequence against `torch.optim.Adam` in float64, bar 1e-12.
  library         every new entry point is declared in the header, bound and exported; the MNF_ERR_INVALID paths that need no device."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import localize_ref as LR

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("mnf_pose_rays", "mnf_pose_loss", "mnf_pose_update", "mnf_pose_refine_workspace_bytes", "mnf_pose_refine_workspace_offset", "mnf_pose_refine")
INVALID = -1


def _rotvec(norm, seed):
    k = np.random.default_rng(seed).standard_normal(3)
    return k / np.linalg.norm(k) * norm


@pytest.mark.parametrize("norm", [0.0, np.sqrt(1e-6) * (1 - 1e-6), np.sqrt(1e-6) * (1 + 1e-6), 0.3, 2.5], ids=["zero", "below", "above", "0.3", "2.5"])
def test_pose_gradient_equals_autograd_through_transform_rays(norm):
    from apnrf_amd import render as RD
    rng = np.random.default_rng(3)
    n = 257
    k = _rotvec(norm, 5)
    assert norm == 0.0 or ((k * k).sum() < 1e-6) == (norm < 1e-3)
    trans = rng.standard_normal(3) * 0.2
    d = rng.standard_normal((n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    centre = rng.standard_normal(3)
    g_o, g_d = rng.standard_normal((n, 3)), rng.standard_normal((n, 3))
    rot_t, tr_t = torch.tensor(k, requires_grad=True), torch.tensor(trans, requires_grad=True)
    rays = RD.transform_rays(RD.Rays(torch.tensor(centre).expand(n, 3).clone(), torch.tensor(d)), rot_t, tr_t)
    assert rays.viewdirs.dtype == torch.float64
    (torch.tensor(g_o) * rays.origins).sum().add((torch.tensor(g_d) * rays.viewdirs).sum()).backward()
    want = np.concatenate([rot_t.grad.numpy(), tr_t.grad.numpy()])
    got, _ = LR.pose_gradient(g_o, g_d, rays.viewdirs.detach().numpy(), k)
    err = np.abs(got - want).max() / np.abs(want).max()
    print(f"|rotvec| = {norm:.6g}: pose gradient rel err {err:.3e} (bar 1e-9)")
    assert err < 1e-9
    # the restated R is transform_rays' R
    R = LR.rodrigues64(k[None])[0]
    assert np.abs(d @ R.T - rays.viewdirs.detach().numpy()).max() < 1e-14


def test_adam_equals_torch_adam_over_20_steps():
    rng = np.random.default_rng(11)
    grads = rng.standard_normal((20, 2, 6)) * np.logspace(-3, 1, 6)[None, None, :]
    grads[7, 1, 2] = 0.0
    lr_rot, lr_trans = 2e-3, 7e-3
    x0 = rng.standard_normal((2, 6)) * 0.1
    rot, tr = torch.tensor(x0[:, :3].copy(), requires_grad=True), torch.tensor(x0[:, 3:].copy(), requires_grad=True)
    opt = torch.optim.Adam([dict(params=[rot], lr=lr_rot), dict(params=[tr], lr=lr_trans)], betas=(0.9, 0.999), eps=1e-15)
    xi, m, v = x0.copy(), np.zeros((2, 6)), np.zeros((2, 6))
    worst = 0.0
    for step in range(20):
        rot.grad, tr.grad = torch.tensor(grads[step, :, :3].copy()), torch.tensor(grads[step, :, 3:].copy())
        opt.step()
        xi, m, v = LR.adam_step(xi, m, v, grads[step], step + 1, lr_rot, lr_trans)
        want = np.concatenate([rot.detach().numpy(), tr.detach().numpy()], 1)
        worst = max(worst, np.abs(xi - want).max())
    print(f"Adam over 20 steps: max abs difference {worst:.3e} (bar 1e-12)")
    assert worst < 1e-12


def test_pose_update_skip_rules_in_the_restatement():
    rng = np.random.default_rng(2)
    B, n = 4, 9
    g_o, g_d, d = (rng.standard_normal((B, n, 3)) for _ in range(3))
    kept = np.ones((B, n), np.int64)
    kept[1] = 0
    status = np.array([0, 0, 8, 0], np.int32)
    xi0 = rng.standard_normal((B, 6)) * 0.1
    xi, m, v, stalled, _ = LR.pose_update(g_o, g_d, d, kept, status, 0, xi0, np.zeros((B, 6)), np.zeros((B, 6)), np.zeros(B), 0, 1e-3, 1e-3)
    assert stalled.tolist() == [0, 1, 1, 0]
    assert (xi[1] == xi0[1]).all() and (xi[2] == xi0[2]).all() and (m[1] == 0).all() and (v[2] == 0).all()
    assert (xi[0] != xi0[0]).all() and (xi[3] != xi0[3]).all()
    _, _, _, stalled, _ = LR.pose_update(g_o, g_d, d, kept, status, 1, xi0, np.zeros((B, 6)), np.zeros((B, 6)), np.zeros(B), 0, 1e-3, 1e-3)
    assert stalled.tolist() == [1, 1, 1, 1]


def test_pixel_draw_is_in_range_and_differs_between_iterations():
    a, b = LR.draw_pixels(3, 193, 0, 42, 37, 23), LR.draw_pixels(3, 193, 1, 42, 37, 23)
    assert a.min() >= 0 and a.max() < 37 * 23 and (a != b).any() and (a[0] != a[1]).any()
    assert len(np.unique(LR.draw_pixels(1, 4096, 0, 1, 64, 64) % 64)) == 64      # every column is reached


def test_header_bindings_and_exports():
    """Fails without the feature: the header declares every new entry point, the binding table has it and the built library exports it."""
    from apnrf_amd import _lib as L
    header = open(os.path.join(REPO, "include", "mi355nerf.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    raw = ctypes.CDLL(L.lib_path())
    for s in SYMBOLS:
        assert re.search(r"\b" + s + r"\s*\(", code), f"{s} is not declared in include/mi355nerf.h"
        assert s in L.SIGNATURES
        assert hasattr(raw, s), f"{s} is not exported by the built library"
    assert L.SIGNATURES["mnf_pose_refine_workspace_bytes"][0] is ctypes.c_int64
    assert len(L.SIGNATURES["mnf_pose_rays"][1]) == 25 and len(L.SIGNATURES["mnf_pose_loss"][1]) == 17
    assert len(L.SIGNATURES["mnf_pose_update"][1]) == 16 and len(L.SIGNATURES["mnf_pose_refine"][1]) == 37
    body = header[header.index("typedef struct mnf_pose_opts_s {"):header.index("} mnf_pose_opts;")]      # the struct the library takes by pointer declares its size first
    assert body.split("\n")[1].strip().startswith("uint32_t struct_size;")
    assert ctypes.sizeof(L.PoseOpts) == 64 and L.PoseOpts().struct_size == 64
    for k, name in enumerate(("RAYS_O", "RAYS_D", "PIX", "RGB", "ACC", "DEPTH", "SEM", "G_RAYS_O", "G_RAYS_D", "GRAD", "ROT", "KEPT")):
        assert re.search(r"#define\s+MNF_POSE_WS_%s\s+%d\b" % (name, k), code), name
    for label in ("pose_rays", "pose_loss", "pose_update"):
        assert f'"{label}"' in header


def test_invalid_arguments_return_before_any_device_call():
    """MNF_ERR_INVALID paths that need no device: null pointers, sizes, a wrong struct_size, misaligned float64 arrays.  Pointers that pass the null checks
    are host addresses nothing dereferences: every check below fails in front of the first HIP call."""
    from apnrf_amd import _lib as L
    lib = L.load_library()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    odd = ctypes.c_void_p(p.value + 4)
    pose = L.PoseOpts()
    pose.w_rgb, pose.w_dep, pose.w_sem, pose.lr_rot, pose.lr_trans, pose.beta1, pose.beta2, pose.eps = 10, 0.2, 0.5, 1e-3, 1e-3, 0.9, 0.999, 1e-15

    def rays(**kw):
        a = dict(images=p, depths=p, f16=0, sems=p, u8=0, n_images=1, ids=p, c2w=p, focal=32.0, W=8, H=8, pix=None, xi=p, B=1, n=4, it=0, seed=0, o=p, d=p,
                 pix_out=p, rot=None, rgb=p, dep=p, lab=p)
        a.update(kw)
        return lib.mnf_pose_rays(*a.values(), None)

    for kw in (dict(images=None), dict(xi=None), dict(o=None), dict(B=0), dict(n=0), dict(B=1 << 16, n=1 << 16), dict(W=0), dict(focal=0.0), dict(n_images=0),
               dict(it=-1), dict(it=1 << 32), dict(xi=odd), dict(pix_out=odd)):
        assert rays(**kw) == INVALID, kw
        assert lib.mnf_last_error().decode().startswith("pose_rays:"), kw

    def loss(pose_=pose, **kw):
        a = dict(rgb=p, depth=p, sem=p, t_rgb=p, t_dep=p, t_lab=p, B=1, n=4, C=3)
        a.update(kw)
        return lib.mnf_pose_loss(*a.values(), ctypes.byref(pose_) if pose_ is not None else None, p, p, p, p, p, None, None)

    short = L.PoseOpts()
    short.struct_size = 48
    bad_beta = L.PoseOpts()
    ctypes.memmove(ctypes.byref(bad_beta), ctypes.byref(pose), ctypes.sizeof(pose))
    bad_beta.beta2 = 1.0
    assert loss(pose_=None) == INVALID and loss(pose_=short) == INVALID and loss(pose_=bad_beta) == INVALID
    for kw in (dict(rgb=None), dict(sem=None), dict(B=0), dict(n=-1), dict(C=-1)):
        assert loss(**kw) == INVALID, kw
    assert "pose_loss" in lib.mnf_last_error().decode()

    def update(**kw):
        a = dict(g_o=p, g_d=p, d=p, kept=None, status=None, skip=None, B=1, n=4, it=0, pose=ctypes.byref(pose), xi=p, m=p, v=p, stalled=p, grad=None)
        a.update(kw)
        return lib.mnf_pose_update(*a.values(), None)

    for kw in (dict(g_o=None), dict(stalled=None), dict(B=0), dict(it=-1), dict(xi=odd), dict(pose=None), dict(pose=ctypes.byref(short))):
        assert update(**kw) == INVALID, kw
    assert lib.mnf_pose_refine_workspace_bytes(None, 1, 4, 100, 100) == -1
    assert lib.mnf_pose_refine_workspace_offset(None, 1, 4, 100, 100, 0) == -1
    opts = L.TrainOpts()
    args = [None, p, None, p, 4, 4, 4, p, p, p, 0, p, 0, 1, p, p, 32.0, 8, 8, None, 1, 4, p, p, p, 0, 1, ctypes.byref(opts), ctypes.byref(pose), p, p, p, 100, 100, p, 1 << 20]
    assert lib.mnf_pose_refine(*args, None) == INVALID      # no field handle
    assert lib.mnf_last_error().decode().startswith("pose_refine:")
