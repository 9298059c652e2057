"""Restatement in numpy / torch float64 of the pose refiner's three stages (csrc/localize.hip, include/mi355nerf.h "pose refinement"), operation by
operation for the fp32 parts.  Inputs and outputs are host arrays.

  draw_pixels     the Philox pixel draw (tests/occ_ref.py's Philox4x32-10, itself held to the published known answers)
  pose_rays       mnf_generate_rays' ray (oracle.render.generate_image_rays, bit-exact against the reference) under the correction, and R rounded once
  targets         mnf_gather_pixels' expressions for B images
  pose_loss       the per-view three-term loss and its plane gradients, with the bad-label rule
  pose_gradient   S_o, S_w and J_l^T S_w in float64
  adam_step       one Adam step on [B,6] with separate learning rates; pose_update adds the skip rules

test_localize_cpu.py holds pose_gradient to float64 autograd through `render.transform_rays` and adam_step to `torch.optim.Adam`."""
import numpy as np
import torch

import occ_ref as OR

PIXEL_TAG = 0x706F7365
SMALL_T2 = 1e-6


def draw_pixels(B, n, iteration, seed, W, H):
    """[B,n] int64: counter (ray, view, iteration, PIXEL_TAG), key (seed low, seed high); x = (u0 W) >> 32, y = (u1 H) >> 32, pix = y W + x"""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    ctr = np.zeros((B, n, 4), np.uint32)
    ctr[..., 0] = np.arange(n, dtype=np.uint32)[None, :]
    ctr[..., 1] = np.arange(B, dtype=np.uint32)[:, None]
    ctr[..., 2] = np.uint32(int(iteration) & 0xFFFFFFFF)
    ctr[..., 3] = np.uint32(PIXEL_TAG)
    w = OR.philox4x32_10(ctr.reshape(-1, 4), np.array([seed & 0xFFFFFFFF, seed >> 32], np.uint32)).astype(np.uint64)
    x = (w[:, 0] * np.uint64(W)) >> np.uint64(32)
    y = (w[:, 1] * np.uint64(H)) >> np.uint64(32)
    return (y * np.uint64(W) + x).astype(np.int64).reshape(B, n)


def rot_coefficients(t2):
    """(a, b, c) of R = I + a K + b K^2 and J_l = I + b K + c K^2 for t^2 (float64 arrays), with the series below SMALL_T2"""
    t2 = np.asarray(t2, np.float64)
    small = t2 < SMALL_T2
    t2s = np.where(small, 1.0, t2)
    t = np.sqrt(t2s)
    a = np.where(small, (1.0 - t2 / 6.0) + t2 * t2 / 120.0, np.sin(t) / t)
    b = np.where(small, (0.5 - t2 / 24.0) + t2 * t2 / 720.0, (1.0 - np.cos(t)) / t2s)
    c = np.where(small, (1.0 / 6.0 - t2 / 120.0) + t2 * t2 / 5040.0, (t - np.sin(t)) / (t2s * t))
    return a, b, c


def rodrigues64(rotvec):
    """[B,3] float64 -> R [B,3,3] float64, entry by entry as the kernel forms them (K^2 = k k^T - t^2 I)"""
    k = np.asarray(rotvec, np.float64).reshape(-1, 3)
    x, y, z = k[:, 0], k[:, 1], k[:, 2]
    t2 = (x * x + y * y) + z * z
    a, b, _ = rot_coefficients(t2)
    R = np.empty((k.shape[0], 3, 3))
    R[:, 0, 0], R[:, 0, 1], R[:, 0, 2] = 1.0 + b * (x * x - t2), -a * z + b * (x * y), a * y + b * (x * z)
    R[:, 1, 0], R[:, 1, 1], R[:, 1, 2] = a * z + b * (x * y), 1.0 + b * (y * y - t2), -a * x + b * (y * z)
    R[:, 2, 0], R[:, 2, 1], R[:, 2, 2] = -a * y + b * (x * z), a * x + b * (y * z), 1.0 + b * (z * z - t2)
    return R


def pose_rays(c2w0, focal, W, H, pix, xi):
    """c2w0 [B,3,4] f32, pix [B,n] int64, xi [B,6] f64 -> (origins [B,n,3] f32, viewdirs [B,n,3] f32, R [B,3,3] f32)"""
    from oracle import render as R_
    f32 = np.float32
    c2w0, xi = np.asarray(c2w0, f32), np.asarray(xi, np.float64)
    B, n = pix.shape
    R = rodrigues64(xi[:, :3]).astype(f32)
    o, d = np.empty((B, n, 3), f32), np.empty((B, n, 3), f32)
    for b in range(B):
        m = np.concatenate([c2w0[b], np.array([[0, 0, 0, 1]], f32)], 0)
        _, d0 = R_.generate_image_rays(m, W, H, focal, np.asarray(pix[b]))
        d0 = d0.numpy().astype(f32)
        for j in range(3):
            d[b, :, j] = (R[b, j, 0] * d0[:, 0] + R[b, j, 1] * d0[:, 1]) + R[b, j, 2] * d0[:, 2]
        o[b] = (c2w0[b, :, 3].astype(np.float64) + xi[b, 3:]).astype(f32)[None, :]
    return o, d, R


def targets(images, depths, sems, image_ids, pix):
    """images [N,H,W,3] u8, depths [N,H,W] f32 | f16, sems [N,H,W] i64 | u8 -> rgb [B,n,3] f32 = u8 / 255.0f, dep [B,n] f32, lab [B,n] i64"""
    B, n = pix.shape
    img = np.asarray(images).reshape(images.shape[0], -1, 3)
    dep = np.asarray(depths).reshape(depths.shape[0], -1)
    sem = np.asarray(sems).reshape(sems.shape[0], -1)
    ids = np.asarray(image_ids).reshape(B, 1)
    return (img[ids, pix].astype(np.float32) / np.float32(255.0)), dep[ids, pix].astype(np.float32), sem[ids, pix].astype(np.int64)


def pose_loss(rgb, depth, sem, t_rgb, t_dep, t_lab, weights=(10.0, 0.2, 0.5)):
    """Planes [B,n,3], [B,n], [B,n,C] and targets -> (loss [B] f64, g_rgb, g_depth, g_sem f64, view_status [B]).  torch float64 autograd per view; a view with
    a label outside [0, C): status 8, zero gradients, the loss over its valid rays only (the mean still over n)."""
    import torch.nn.functional as F
    B, n, C = sem.shape
    loss, status = np.zeros(B), np.zeros(B, np.int32)
    g = [np.zeros(rgb.shape), np.zeros(depth.shape), np.zeros(sem.shape)]
    for b in range(B):
        planes = [torch.tensor(np.asarray(x[b], np.float64), requires_grad=True) for x in (rgb, depth, sem)]
        lab = torch.from_numpy(np.asarray(t_lab[b], np.int64))
        ok = (lab >= 0) & (lab < C)
        l_rgb = F.smooth_l1_loss(planes[0], torch.tensor(np.asarray(t_rgb[b], np.float64)))
        l_dep = F.smooth_l1_loss(planes[1], torch.tensor(np.asarray(t_dep[b], np.float64)))
        l_sem = F.cross_entropy(planes[2][ok], lab[ok], reduction="sum") / n
        total = weights[0] * l_rgb + weights[1] * l_dep + weights[2] * l_sem
        loss[b] = float(total.detach())
        if bool(ok.all()):
            for k, gk in enumerate(torch.autograd.grad(total, planes)):
                g[k][b] = gk.numpy()
        else:
            status[b] = 8
    return loss, g[0], g[1], g[2], status


def pose_gradient(g_o, g_d, d, rotvec):
    """One view: g_o, g_d, d [n,3] (any float dtype, taken to float64), rotvec [3] -> (grad [6] f64 = (dL/drotvec, dL/dtrans), terms [6]: the sums of the
    absolute values of what was added, for error bars)"""
    g_o, g_d, d, k = (np.asarray(x, np.float64) for x in (g_o, g_d, d, rotvec))
    S_o, S_w = g_o.sum(0), np.cross(d, g_d).sum(0)
    _, b, c = rot_coefficients(np.array((k * k).sum()))
    kx = np.cross(k, S_w)
    g_rot = S_w - b * kx + c * np.cross(k, kx)
    terms_w = (np.abs(d[:, [1, 2, 0]] * g_d[:, [2, 0, 1]]) + np.abs(d[:, [2, 0, 1]] * g_d[:, [1, 2, 0]])).sum(0)
    return np.concatenate([g_rot, S_o]), np.concatenate([terms_w, np.abs(g_o).sum(0)])


def adam_step(xi, m, v, g, step, lr_rot, lr_trans, beta1=0.9, beta2=0.999, eps=1e-15):
    """One Adam step (bias-corrected moments, step = 1, 2, ...) on float64 [.., 6]; returns new (xi, m, v)"""
    xi, m, v, g = (np.asarray(x, np.float64) for x in (xi, m, v, g))
    lr = np.array([lr_rot] * 3 + [lr_trans] * 3)
    m = beta1 * m + (1.0 - beta1) * g
    v = beta2 * v + (1.0 - beta2) * (g * g)
    bc1, bc2s = 1.0 - beta1 ** step, np.sqrt(1.0 - beta2 ** step)
    return xi - (lr / bc1) * (m / (np.sqrt(v) / bc2s + eps)), m, v


def pose_update(g_o, g_d, d, kept, view_status, skip, xi, m, v, stalled, iteration, lr_rot, lr_trans, **adam_kw):
    """B views: arrays [B,n,3], kept [B,n] or None, view_status [B] or None, skip scalar -> new (xi, m, v, stalled, grad [B,6])"""
    xi, m, v, stalled = np.array(xi, np.float64), np.array(m, np.float64), np.array(v, np.float64), np.array(stalled, np.int64)
    grad = np.zeros_like(xi)
    for b in range(xi.shape[0]):
        grad[b], _ = pose_gradient(g_o[b], g_d[b], d[b], xi[b, :3])
        stall = (kept is not None and not (np.asarray(kept[b]) > 0).any()) or (view_status is not None and view_status[b] != 0) or skip > 0 \
            or not np.isfinite(grad[b]).all()
        if stall:
            stalled[b] += 1
            continue
        xi[b], m[b], v[b] = adam_step(xi[b], m[b], v[b], grad[b], iteration + 1 - stalled[b], lr_rot, lr_trans, **adam_kw)
    return xi, m, v, stalled, grad
