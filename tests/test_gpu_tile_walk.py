"""The field kernel's tile walk changes no sample's bits: a sample's result depends on neither its tile nor its neighbours, so the first n rows of one
call at n = 4097 are the rows of a call at n, bit for bit.  The sizes cover one lane, one full tile, one lane into a second tile (1, 64, 65), two
workgroups on the plain stride (513: 9 tiles), eight workgroups on the XCD-eighth order (4096: 64 tiles) and nine workgroups back on the plain stride
(4097).  The ticket order and the ray-major walk have their own tests (tests/diag_tile_order.py, test_ray_major_density_prepass_*)."""
import numpy as np
import pytest
import torch

import helpers as H

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N_ALL = 4097
SIZES = [1, 64, 65, 513, 4096, 4097]
_CASES = {}


def _case(neurons, layers):
    """The field of one shape, its inputs, and the outputs of the three entry points at n = 4097: computed once per shape, never modified."""
    key = (neurons, layers)
    if key not in _CASES:
        sc = H.make_scene(neurons=neurons, layers=layers, C=3, log2_hashmap_size=12, head_gain=2.0)
        f = H.hip_field(sc)
        rng = np.random.default_rng(5)
        a = sc["aabb"]
        pos = (rng.random((N_ALL, 3)) * (a[3:] - a[:3]) * 0.98 + a[:3] + 0.01 * (a[3:] - a[:3])).astype(np.float32)
        pos[::97] = a[:3] - 1.0                                          # a few positions outside the box
        d = rng.normal(size=(N_ALL, 3)).astype(np.float32); d /= np.linalg.norm(d, axis=-1, keepdims=True)
        pos, d = torch.from_numpy(pos).to(DEV), torch.from_numpy(d).to(DEV)
        # the same points as rays: one ray per sample, the point at the middle of its interval
        ts = torch.from_numpy(rng.uniform(0.5, 0.9, N_ALL).astype(np.float32)).to(DEV)
        te = ts + 0.25
        o = pos - d * ((ts + te) / 2)[:, None]
        ri = torch.arange(N_ALL, device=DEV, dtype=torch.int64)
        with torch.no_grad():
            full = dict(forward=f(pos, d), density=f.query_density(pos), samples=f.forward_samples(o, d, ri, ts, te))
        _CASES[key] = (f, pos, d, o, ri, ts, te, full)
    return _CASES[key]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("neurons,layers", [(128, 2), (64, 1)])
def test_tile_walk_changes_no_bits(neurons, layers, n):
    f, pos, d, o, ri, ts, te, full = _case(neurons, layers)
    with torch.no_grad():
        got = dict(forward=f(pos[:n], d[:n]), density=f.query_density(pos[:n]), samples=f.forward_samples(o, d, ri[:n], ts[:n], te[:n]))
    for name in ("forward", "density", "samples"):
        want, have = full[name], got[name]
        if torch.is_tensor(want):
            want, have = (want,), (have,)
        for k, (w, g) in enumerate(zip(want, have)):
            assert g.shape[0] == n
            assert torch.equal(g, w[:n]), f"{name} output {k} at n = {n} differs from the first rows of the call at n = {N_ALL}"
    assert float(full["density"].max()) > 0.0 and bool(torch.isfinite(full["forward"][0]).all())
