"""The two closed forms `field_input_grad_kernel` (csrc/inputgrad.hip) implements, restated in numpy and held against torch autograd of the
oracle's own encodings: the 16 x 3 Jacobian of the degree-4 spherical harmonics and the per-level derivative of the trilinear hash blend."""
import numpy as np
import torch

import helpers as H
from oracle.field import PRIMES, OracleField

C1, C2, C3, C5 = 0.48860251190291987, 1.0925484305920792, 0.94617469575755997, 0.54627421529603959
C6, C7, C8, C9, C10 = 0.59004358992664352, 2.8906114426405538, 0.45704579946446572, 0.3731763325901154, 1.4453057213202769


def sh4_jacobian(d):
    """[N,3] directions -> [N,16,3]: d(sh4)/d(x, y, z) of oracle/field.py:231-256 at (x, y, z) = d (the map d -> (d+1)/2 -> 2u-1 is the identity)."""
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    x2, y2, z2 = x * x, y * y, z * z
    o, zero = np.ones_like(x), np.zeros_like(x)
    rows = [
        (zero, zero, zero),
        (zero, -C1 * o, zero),
        (zero, zero, C1 * o),
        (-C1 * o, zero, zero),
        (C2 * y, C2 * x, zero),
        (zero, -C2 * z, -C2 * y),
        (zero, zero, 2 * C3 * z),
        (-C2 * z, zero, -C2 * x),
        (2 * C5 * x, -2 * C5 * y, zero),
        (-6 * C6 * x * y, 3 * C6 * (y2 - x2), zero),
        (C7 * y * z, C7 * x * z, C7 * x * y),
        (zero, C8 * (1 - 5 * z2), -10 * C8 * y * z),
        (zero, zero, C9 * (15 * z2 - 3)),
        (C8 * (1 - 5 * z2), zero, -10 * C8 * x * z),
        (2 * C10 * x * z, -2 * C10 * y * z, C10 * (x2 - y2)),
        (3 * C6 * (y2 - x2), 6 * C6 * x * y, zero),
    ]
    return np.stack([np.stack(r, -1) for r in rows], 1)


def hash_position_gradient(orc, xn, g):
    """dL/dxn [N,3] from g = dL/d(features) [N,64]: per level scale * sum_{by,bz} wy wz dot(g_l, e(1,by,bz) - e(0,by,bz)), likewise y and z, with the
    cells, fractions and entries of the forward (fractions in fp32 as the forward forms them, the sums in float64)."""
    table = orc.table.detach().numpy().astype(np.float64)
    out = np.zeros((xn.shape[0], 3))
    for l, lv in enumerate(orc.levels):
        pos = (xn.astype(np.float64) * float(lv["scale"]) + 0.5).astype(np.float32)
        cell = np.floor(pos)
        frac = (pos - cell).astype(np.float64)
        cell = cell.astype(np.int32).astype(np.int64) & 0xFFFFFFFF
        e = np.zeros((2, 2, 2, xn.shape[0], 4))
        for bx in range(2):
            for by in range(2):
                for bz in range(2):
                    c = [(cell[:, 0] + bx) & 0xFFFFFFFF, (cell[:, 1] + by) & 0xFFFFFFFF, (cell[:, 2] + bz) & 0xFFFFFFFF]
                    if lv["hashed"]:
                        idx = (((c[0] * PRIMES[0]) & 0xFFFFFFFF) ^ ((c[1] * PRIMES[1]) & 0xFFFFFFFF) ^ ((c[2] * PRIMES[2]) & 0xFFFFFFFF)) % lv["n"]
                    else:
                        idx = ((c[0] + c[1] * lv["res"] + c[2] * lv["res"] ** 2) & 0xFFFFFFFF) % lv["n"]
                    e[bx, by, bz] = table[lv["offset"] + idx]
        gl = g[:, 4 * l:4 * l + 4].astype(np.float64)
        D = (e * gl).sum(-1)                                              # [bx,by,bz,N] = dot(g, entry)
        w = np.stack([1.0 - frac, frac])                                  # [bit,N,axis]
        gx = sum(w[by, :, 1] * w[bz, :, 2] * (D[1, by, bz] - D[0, by, bz]) for by in range(2) for bz in range(2))
        gy = sum(w[bx, :, 0] * w[bz, :, 2] * (D[bx, 1, bz] - D[bx, 0, bz]) for bx in range(2) for bz in range(2))
        gz = sum(w[bx, :, 0] * w[by, :, 1] * (D[bx, by, 1] - D[bx, by, 0]) for bx in range(2) for by in range(2))
        out += float(lv["scale"]) * np.stack([gx, gy, gz], -1)
    return out


def _rel(got, want):
    return float(np.linalg.norm(got - want) / np.linalg.norm(want))


def test_closed_forms_match_oracle_autograd():
    rng = np.random.default_rng(3)
    n = 192
    # spherical harmonics (float64 on both sides: the formulas, not fp32 rounding, are under test)
    d = rng.normal(size=(n, 3)); d /= np.linalg.norm(d, axis=-1, keepdims=True)
    g_sh = rng.normal(size=(n, 16))
    dt = torch.from_numpy(d).requires_grad_()
    (OracleField.sh4((dt + 1.0) / 2.0) * torch.from_numpy(g_sh)).sum().backward()
    got = np.einsum("nk,nkc->nc", g_sh, sh4_jacobian(d))
    err = _rel(got, dt.grad.numpy())
    print(f"SH Jacobian: rel L2 {err:.3e}")
    assert err < 1e-6
    # hash blend at two table sizes (dense and hashed levels in both), positions outside the unit box included (the dense levels wrap, the hash does not care)
    for lh in (12, 15):
        sc = H.make_scene(neurons=64, layers=2, C=5, log2_hashmap_size=lh)
        orc = H.oracle_field(sc)
        xn = rng.random((n, 3)).astype(np.float32)
        xn[:5] = rng.random((5, 3)).astype(np.float32) * 0.3 - 0.4
        g = rng.normal(size=(n, 64)).astype(np.float32)
        xt = torch.from_numpy(xn).requires_grad_()
        (orc.hash_encode(xt) * torch.from_numpy(g)).sum().backward()
        want = xt.grad.numpy().astype(np.float64)
        err = _rel(hash_position_gradient(orc, xn, g), want)
        print(f"hash levels (log2 T = {lh}): rel L2 {err:.3e}, max |dL/dxn| {np.abs(want).max():.3e}")
        assert err < 1e-6
