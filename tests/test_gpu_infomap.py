"""GPU tests of the per-pixel predictive-information maps: `mnf_score_view_maps` (csrc/infomap.hip) through
`render.view_information_maps` and through the raw entry point, and the whole route `render.score_view_maps`.

The yardstick is tests/infomap_ref.py: the four per-pixel terms of scripts/pipeline.py:727-774 in numpy float64, which
test_infomap_cpu.py pins to the RUNNING reference's recorded scorer at 1e-12.  Bars:

  * maps and terms against the restatement: 1e-9 absolute, the project's bar for scorer terms.  The kernel works in
    float64 on the same widened fp32 inputs; what differs is the last bits of exp / log and the order of sums of at most 1024 classes
    and 64 members, of the order of 1e-13.
  * terms against the mean of the kernel's own maps: the worst-case float64 summation bound P * 2^-53 * max|map| of the view's column.
  * heat bytes against the restatement's scaling applied in numpy to the kernel's own float64 maps: equality.  The operations and their
    order are specified and every one is rounded on its own, so no tie allowance is needed.
  * offsets, batches and repeats: equality of bits."""
import functools
import os

import numpy as np
import pytest
import torch

import helpers as H
import infomap_ref as IR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN, INF = float("nan"), float("inf")
GUARD = 0xA5
ATOL = 1e-9
GOLDEN = (2, 40, 25, 29)
# (M, V, P, C): the golden's own stacks; the smallest case; at 29 classes a tile is 184 pixels, so 255 and 257 are two tiles, the second
# short; M = 3: the / 2 of pipeline.py:733 is not / M; C = 33: above score_kernel's class limit, M = 5 above its unrolled form; C = 64:
# padded rows, tiles of 80; the member maximum; the class maximum (tiles of 4 pixels); 514 tiles of 256 pixels per view: runs of two tiles
SHAPES = [GOLDEN, (1, 1, 1, 1), (2, 3, 255, 29), (2, 2, 257, 29), (3, 2, 300, 32), (5, 1, 64, 33), (2, 1, 513, 64), (64, 1, 70, 7), (2, 1, 40, 1024),
          (2, 2, 131372, 3)]
IDS = lambda s: "M{}_V{}_P{}_C{}".format(*s)
HEAT_LO, HEAT_HI = (-0.05, 0.9, -0.01, -0.02), (0.6, -0.05, 0.4, 0.3)        # the depth ramp is reversed


def _cu(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)          # a copy: the shared stacks are read-only


def make_stacks(M, V, P, C, seed):
    """Seeded fp32 stacks: variances mixing exact 0, 1e-8 and O(1); opacities mixing 0, 1, 1 + 2.4e-7 (legal: the golden holds one) and
    uniform; logits scaled 0.1, 5 and 50 pixel by pixel."""
    rng = np.random.default_rng(seed)
    def variance(shape):
        x = rng.random(shape) ** 4
        pick = rng.integers(0, 4, shape)
        return np.where(pick == 0, 0.0, np.where(pick == 1, 1e-8, x)).astype(np.float32)
    rv, dv = variance((M, V, P, 3)), variance((M, V, P))
    pick = rng.integers(0, 6, (M, V, P))
    ac = np.select([pick == 0, pick == 1, pick == 2], [0.0, 1.0, 1.0 + 2.4e-7], rng.random((M, V, P))).astype(np.float32)
    scale = np.array([0.1, 5.0, 50.0])[rng.integers(0, 3, (M, V, P, 1))]
    sm = (rng.standard_normal((M, V, P, C)) * scale).astype(np.float32)
    return rv, dv, ac, sm


def golden_stacks():
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scorer.npz"))
    st = lambda nm, tail: np.stack([g[f"m{m}_{nm}"].astype(np.float32) for m in range(2)]).reshape(2, 40, 25, *tail)
    return st("images_var", (3,)), st("depths_var", ()), st("accs", ()), st("sems", (29,))


@functools.lru_cache(maxsize=None)
def case(shape):
    """(stacks, the restatement's maps) of a shape: made once, shared by the tests, never written to."""
    M, V, P, C = shape
    stacks = golden_stacks() if shape == GOLDEN else make_stacks(M, V, P, C, seed=M + 7 * V + P + 31 * C)
    assert stacks[3].shape == shape
    for a in stacks:
        a.setflags(write=False)
    ref = IR.maps(*stacks)
    ref.setflags(write=False)
    return stacks, ref


@functools.lru_cache(maxsize=None)
def kernel(shape):
    """(terms, maps, heat) of `view_information_maps` on a shape's stacks, as host arrays."""
    from apnrf_amd import render as RD
    stacks, _ = case(shape)
    terms, maps, heat = RD.view_information_maps(*(_cu(a) for a in stacks), heat_range=(HEAT_LO, HEAT_HI))
    M, V, P, C = shape
    assert terms.shape == (V, 4) and maps.shape == (V, P, 4) and heat.shape == (V, P, 4)
    assert terms.dtype == torch.float64 and maps.dtype == torch.float64 and heat.dtype == torch.uint8 and heat.is_cuda
    return terms.cpu().numpy(), maps.cpu().numpy(), heat.cpu().numpy()


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_maps_and_terms_match_restatement(shape):
    _, ref = case(shape)
    terms, maps, _ = kernel(shape)
    assert np.isfinite(ref).all() and np.isfinite(maps).all()
    print(f"{shape}: max |maps - ref| = {np.abs(maps - ref).max():.3e}, max |terms - ref| = {np.abs(terms - IR.terms_of_maps(ref)).max():.3e}, "
          f"max |ref| = {np.abs(ref).max():.3f}")
    np.testing.assert_allclose(maps, ref, rtol=0, atol=ATOL)
    np.testing.assert_allclose(terms, IR.terms_of_maps(ref), rtol=0, atol=ATOL)


def test_golden_terms_are_the_references_own(golden):
    g = golden("scorer")
    terms, maps, _ = kernel(GOLDEN)
    np.testing.assert_allclose(terms.mean(0) * IR.WEIGHTS, g["terms"], rtol=0, atol=ATOL)
    np.testing.assert_allclose(maps.reshape(-1, 4).mean(0) @ IR.WEIGHTS, float(g["pi"]), rtol=0, atol=ATOL)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_terms_are_the_means_of_the_maps(shape):
    P = shape[2]
    terms, maps, _ = kernel(shape)
    bound = P * 2.0 ** -53 * np.abs(maps).max(axis=1)            # [V,4]; column 0 of the maps is the per-pixel channel mean
    err = np.abs(terms - maps.mean(axis=1))
    print(f"{shape}: |terms - mean(maps)| / bound = {(err / np.maximum(bound, 1e-300)).max():.3f}")
    assert (err <= bound).all(), (err, bound)


@pytest.mark.parametrize("shape", [s for s in SHAPES if s[3] <= 32], ids=IDS)
def test_terms_match_score_views(shape):
    from apnrf_amd import render as RD
    stacks, _ = case(shape)
    terms, _, _ = kernel(shape)
    old = RD.score_view_terms(*(_cu(a) for a in stacks)).cpu().numpy()
    print(f"{shape}: max |terms - mnf_score_views| = {np.abs(terms - old).max():.3e}")
    np.testing.assert_allclose(terms, old, rtol=0, atol=ATOL)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_heat_bytes_are_the_scaled_maps(shape):
    _, maps, heat = kernel(shape)
    want = IR.heat(maps, HEAT_LO, HEAT_HI)
    bad = np.argwhere(heat != want)
    assert bad.size == 0, f"{len(bad)} bytes differ, first {bad[0].tolist()}: got {heat[tuple(bad[0])]} want {want[tuple(bad[0])]} for {maps[tuple(bad[0])]!r}"
    if shape[0] == 2 and shape[2] >= 255:
        assert len(np.unique(heat)) > 32                          # a ramp, not a constant (64 members saturate the rgb and depth ranges)


def test_outputs_are_optional():
    from apnrf_amd import render as RD
    shape = (2, 2, 257, 29)
    dev = [_cu(a) for a in case(shape)[0]]
    terms, maps, heat = kernel(shape)
    t, m, h = RD.view_information_maps(*dev, maps=False)
    assert m is None and h is None and np.array_equal(t.cpu().numpy(), terms)
    t, m, h = RD.view_information_maps(*dev)
    assert h is None and np.array_equal(t.cpu().numpy(), terms) and np.array_equal(m.cpu().numpy(), maps)
    t, m, h = RD.view_information_maps(*dev, maps=False, heat_range=(HEAT_LO, HEAT_HI))
    assert m is None and np.array_equal(t.cpu().numpy(), terms) and np.array_equal(h.cpu().numpy(), heat)
    with pytest.raises(ValueError, match="do not match"):
        RD.view_information_maps(dev[0], dev[1][:, :, :-1], dev[2], dev[3])


def test_identical_members_carry_no_information():
    from apnrf_amd import render as RD
    one = [a[:1] for a in make_stacks(1, 2, 300, 29, seed=5)]
    terms, maps, _ = RD.view_information_maps(*(_cu(np.repeat(a, 2, axis=0)) for a in one))
    print(f"identical members: max |map| = {maps.abs().max().item():.3e}, max |term| = {terms.abs().max().item():.3e}")
    assert maps.abs().max().item() <= ATOL and terms.abs().max().item() <= ATOL


def test_nan_and_inf_stay_in_their_view():
    from apnrf_amd import render as RD
    shape = (2, 3, 255, 29)
    stacks, _ = case(shape)
    clean_terms, clean_maps, clean_heat = kernel(shape)
    rv, dv, ac, sm = (a.copy() for a in stacks)
    rv[1, 1, 17, 2] = NAN; dv[0, 1, 17] = NAN; ac[1, 1, 17] = NAN; sm[0, 1, 17, 3] = NAN       # a NaN pixel
    sm[1, 1, 200, 28] = INF                                                                    # an inf logit (second tile)
    ref = IR.maps(rv, dv, ac, sm)
    terms, maps, heat = RD.view_information_maps(_cu(rv), _cu(dv), _cu(ac), _cu(sm), heat_range=(HEAT_LO, HEAT_HI))
    terms, maps, heat = terms.cpu().numpy(), maps.cpu().numpy(), heat.cpu().numpy()
    assert np.isnan(ref[1, 17]).all() and np.isnan(ref[1, 200]).tolist() == [False, False, True, False] and np.isnan(ref).sum() == 5
    assert np.array_equal(np.isnan(maps), np.isnan(ref))
    np.testing.assert_allclose(np.nan_to_num(maps, nan=0.0), np.nan_to_num(ref, nan=0.0), rtol=0, atol=ATOL)
    assert np.isnan(terms).tolist() == [[False] * 4, [True] * 4, [False] * 4]
    assert (heat[1, 17] == 0).all() and heat[1, 200, 2] == 0                   # NaN -> 0
    for v in (0, 2):                                                             # the other views keep their bits
        assert np.array_equal(terms[v], clean_terms[v]) and np.array_equal(maps[v], clean_maps[v]) and np.array_equal(heat[v], clean_heat[v])
    ok = ~np.isnan(ref[1]).any(axis=1)
    assert np.array_equal(maps[1][ok], clean_maps[1][ok]) and np.array_equal(heat[1][ok], clean_heat[1][ok])


# ------------------------------------------------------------------ the raw entry point: offsets and guard bytes
def _dev_ptr(addr):
    from apnrf_amd import _lib as L
    p = L.DevPtr(addr)
    p.device = torch.device(DEV)
    return p


def _raw(stacks, in_off=0, maps_off=0, heat_off=0, want=("terms", "maps", "heat")):
    """mnf_score_view_maps with every input `in_off` floats into its allocation and every output inside a buffer pre-filled with 0xA5
    (maps `maps_off` bytes and heat `heat_off` bytes past a 64-byte pad).  Returns the outputs after checking the guard bytes."""
    import ctypes
    from apnrf_amd import _lib as L
    lib = L.load_library()
    M, V, P, C = stacks[3].shape
    ins = []
    for a in stacks:
        big = torch.empty(a.size + in_off, dtype=torch.float32, device=DEV)
        big[in_off:] = _cu(a).reshape(-1)
        assert big.data_ptr() % 16 == 0
        ins.append(big)
    pad = 64
    spec = dict(terms=(V * 4 * 8, 0), maps=(V * P * 4 * 8, maps_off), heat=(V * P * 4, heat_off))
    bufs = {k: torch.full((pad + off + n + pad,), GUARD, dtype=torch.uint8, device=DEV) for k, (n, off) in spec.items()}
    assert all(b.data_ptr() % 16 == 0 for b in bufs.values())
    ptrs = {k: (_dev_ptr(bufs[k].data_ptr() + pad + spec[k][1]) if k in want else None) for k in spec}
    nbytes = max(int(lib.mnf_score_view_maps_workspace_bytes(V, P, C)), 8)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    lo, hi = (ctypes.c_double * 4)(*HEAT_LO), (ctypes.c_double * 4)(*HEAT_HI)
    L.launch(lib.mnf_score_view_maps, *[_dev_ptr(t.data_ptr() + 4 * in_off) for t in ins], M, V, P, C, ptrs["terms"], ptrs["maps"], ptrs["heat"],
             lo if "heat" in want else None, hi if "heat" in want else None, L.ptr(ws), nbytes)
    out = {}
    for k, (n, off) in spec.items():
        host = bufs[k].cpu().numpy()
        if k not in want:
            assert (host == GUARD).all(), f"{k} was skipped but its buffer was written"
            continue
        assert (host[:pad + off] == GUARD).all(), f"{k}: a byte before the output was written"
        assert (host[pad + off + n:] == GUARD).all(), f"{k}: a byte after the output was written"
        body = host[pad + off:pad + off + n].copy()
        out[k] = body.reshape(V, P, 4) if k == "heat" else body.view(np.float64).reshape((V, 4) if k == "terms" else (V, P, 4))
    return out


@pytest.mark.parametrize("off", [0, 1, 2, 3])
def test_unaligned_inputs_and_guarded_outputs(off):
    """Inputs 0 - 3 floats into their allocations (a scalar head up to the first 16-byte boundary, 16-byte loads, a scalar tail, from 1 on), maps 8 bytes off the 16-byte grid for odd offsets
    (four 8-byte stores), heat 4 bytes times the offset past its pad: the bits of the aligned call, and no guard byte changes."""
    for shape in [(2, 2, 257, 29), (3, 2, 300, 32)]:              # odd and even class counts: plain and padded LDS rows
        stacks, _ = case(shape)
        terms, maps, heat = kernel(shape)
        got = _raw(stacks, in_off=off, maps_off=8 * (off & 1), heat_off=4 * off)
        assert np.array_equal(got["terms"], terms) and np.array_equal(got["maps"], maps) and np.array_equal(got["heat"], heat), (shape, off)


def test_skipped_outputs_stay_untouched():
    shape = (2, 2, 257, 29)
    stacks, _ = case(shape)
    terms, maps, heat = kernel(shape)
    assert np.array_equal(_raw(stacks, want=("maps",))["maps"], maps)
    assert np.array_equal(_raw(stacks, want=("heat",), heat_off=4)["heat"], heat)
    assert np.array_equal(_raw(stacks, want=("terms",))["terms"], terms)


def test_a_view_alone_in_a_batch_and_repeated():
    from apnrf_amd import render as RD
    for shape in [(2, 3, 255, 29), (2, 2, 131372, 3)]:
        stacks, _ = case(shape)
        terms, maps, heat = kernel(shape)
        dev = [_cu(a) for a in stacks]
        again = RD.view_information_maps(*dev, heat_range=(HEAT_LO, HEAT_HI))
        assert all(np.array_equal(a.cpu().numpy(), b) for a, b in zip(again, (terms, maps, heat)))
        v = shape[1] - 1
        alone = RD.view_information_maps(*(t[:, v:v + 1] for t in dev), heat_range=(HEAT_LO, HEAT_HI))
        assert all(np.array_equal(a.cpu().numpy()[0], b[v]) for a, b in zip(alone, (terms, maps, heat)))
        # the same view twice over in a larger batch, at another position
        more = RD.view_information_maps(*(torch.cat([t[:, v:v + 1], t, t[:, v:v + 1]], dim=1) for t in dev), heat_range=(HEAT_LO, HEAT_HI))
        for a, b in zip(more, (terms, maps, heat)):
            a = a.cpu().numpy()
            assert np.array_equal(a[0], b[v]) and np.array_equal(a[-1], b[v]) and np.array_equal(a[1:-1], b)


# ------------------------------------------------------------------ end to end
def test_score_view_maps_end_to_end():
    from apnrf_amd import render as RD
    scene = H.make_scene()
    sc2 = dict(scene); sc2["params"] = H.S.make_field_params(seed=1)
    fields = [H.hip_field(scene), H.hip_field(sc2)]
    ests = [H.hip_estimator(scene), H.hip_estimator(scene)]
    poses = scene["poses"][[1, 4, 6]]
    args = (fields, ests, poses, 640, 640, 320.0, 0.1, 1e-3, 0.025, 0.004, 0.01, DEV)
    terms_old, score_old = RD.score_views(*args, group=False)
    out = RD.score_view_maps(*args, heat_range=(HEAT_LO, HEAT_HI))
    assert out["maps"].shape == (3, 16, 16, 4) and out["heat"].shape == (3, 16, 16, 4) and out["terms"].shape == (3, 4)
    assert torch.isfinite(out["maps"]).all() and out["maps"].abs().max().item() > 1e-3               # not an empty render
    print(f"end to end: max |terms - score_views| = {(out['terms'] - terms_old).abs().max().item():.3e}")
    np.testing.assert_allclose(out["terms"].cpu().numpy(), terms_old.cpu().numpy(), rtol=0, atol=ATOL)
    assert abs(float(out["score"]) - float(score_old)) <= 7 * ATOL                                   # the weights sum to 7
    assert float(out["score"]) == float(RD.trajectory_score(out["terms"]))
    maps = out["maps"].cpu().numpy()
    assert (np.abs(out["terms"].cpu().numpy() - maps.reshape(3, 256, 4).mean(1)) <= 256 * 2.0 ** -53 * np.abs(maps).reshape(3, 256, 4).max(1)).all()
    assert np.array_equal(out["heat"].cpu().numpy(), IR.heat(maps, HEAT_LO, HEAT_HI))
    for per in (1, 2):
        part = RD.score_view_maps(*args, heat_range=(HEAT_LO, HEAT_HI), views_per_call=per)
        assert all(torch.equal(part[k], out[k]) for k in ("terms", "score", "maps", "heat")), per
    assert RD.score_view_maps(*args)["heat"] is None
