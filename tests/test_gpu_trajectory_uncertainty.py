"""The ensemble-disagreement trajectory scorer on the device: `mnf_score_ensemble_views` (csrc/ensemble.hip), `mnf_score_trajectory`
(csrc/score.hip) and their Python routes `render.ensemble_view_terms` / `render.trajectory_uncertainty`, against

  * the RUNNING reference (`ActiveNeRFMapper.trajector_uncertainty`, scripts/pipeline.py:800-916; tests/golden/trajectory.npz), and
  * the float64 numpy restatement of test_trajectory_uncertainty_cpu.py, which that golden pins to 1e-12,

at rtol = atol = 1e-9: the bar `mnf_score_views` meets on scorer.npz.  The kernel's sums are fp64 sums of at most 4096 terms of fp64
values from the same widened fp32 inputs, so its rounding error is of the order of 1e-13 relative; the atol is for rows that are exactly 0."""

import numpy as np
import pytest
import torch

import helpers as H
from test_glue_golden_cpu import scene_of
from test_trajectory_uncertainty_cpu import ensemble_rows, golden_stacks

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BAR = dict(rtol=1e-9, atol=1e-9)


def _cu(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(DEV)


def _hip_estimator(sc):
    from apnrf_amd.nerfacc import OccGridEstimator
    est = OccGridEstimator(torch.from_numpy(sc["aabb"]), resolution=sc["res"], levels=1)
    est.binaries = torch.from_numpy(sc["occ"])
    est.occs = torch.from_numpy(sc["occs"])
    return est.to(DEV).eval()


def _hip_ngp_field(g, seed):
    from apnrf_amd import synthetic as S
    lh = int(g["log2_hashmap_size"])
    params = S.make_field_params(128, 2, 29, seed=int(seed), log2_hashmap_size=lh)
    return H.hip_field(dict(aabb=g["aabb"], neurons=128, layers=2, C=29, log2_hashmap_size=lh, params=params))


def _terms(stacks):
    from apnrf_amd import render as RD
    return RD.ensemble_view_terms(*stacks).cpu().numpy()


# ------------------------------------------------------------------ 1. the kernel against the reference's own run
def test_kernel_equals_running_reference_on_its_own_stacks(golden):
    g = golden("trajectory")
    rgb, depth, acc, sem = golden_stacks(g)                              # M = 2, V = 40, P = 25, C = 29, S = 1
    t = _terms((_cu(rgb), _cu(depth), _cu(acc), _cu(sem)))
    assert t.shape == (40, 4) and t.dtype == np.float64
    np.testing.assert_allclose(t, g["rows"].T, **BAR)
    t3 = _terms((_cu(rgb), _cu(depth), _cu(acc), _cu(sem[0])))           # sem [V,P,C]: member 0's logits as the reference keeps them
    np.testing.assert_array_equal(t3, t)


# ------------------------------------------------------------------ 2. the kernel against the restatement on synthetic stacks
# (P, C, M, S, V, logit scale): every pair of values of two different parameters occurs in some case (greedy pairwise cover, S <= M).
# P: one lane, part of a wave, 63 / 65 around a wave, 1025 and 4096 more than one workgroup per view (a tile is at most 256 pixels);
# C: 33 and 64 are past any 32-wide scratch, and 1, 29, 33 are odd (LDS row stride C) where 64 is even (stride 65);
# M: 1 gives variance exactly 0, 3 and 5 are past any unrolled member count.
CASES = [
    (1, 1, 1, 1, 1, 0.05), (1, 29, 3, 1, 1, 1), (1, 33, 5, 1, 1, 8), (1, 64, 2, 2, 3, 60),
    (25, 1, 2, 2, 3, 1), (25, 1, 3, 1, 1, 0.05), (25, 29, 1, 1, 1, 60), (25, 33, 5, 1, 1, 0.05), (25, 64, 1, 1, 1, 8),
    (63, 1, 5, 2, 1, 8), (63, 1, 1, 1, 1, 60), (63, 29, 3, 1, 3, 8), (63, 33, 2, 1, 1, 1), (63, 64, 1, 1, 1, 0.05),
    (65, 1, 5, 1, 1, 60), (65, 29, 2, 1, 1, 0.05), (65, 33, 3, 2, 1, 60), (65, 33, 1, 1, 3, 1), (65, 64, 1, 1, 1, 8),
    (1025, 1, 3, 2, 3, 0.05), (1025, 29, 1, 1, 1, 8), (1025, 33, 2, 1, 1, 60), (1025, 64, 5, 1, 1, 1),
    (4096, 1, 1, 1, 1, 60), (4096, 29, 5, 2, 3, 0.05), (4096, 33, 2, 1, 1, 8), (4096, 64, 3, 1, 1, 1),
    (65, 29, 2, 2, 3, 1e4),          # logits at +-1e4: the softmax must subtract the maximum
]
# the accumulation plane cycles through these before the random rest: exact 0 and exact 1, values below 1e-4 of either sign (a negative
# one is the only way past the upper clip end: acc = 0 gives 1 / 1e-4 - 1 = 9999 < 10000), 1 + 1e-3 (below the lower clip end, as 1 is)
ACC_PLANTED = (0.0, 1.0, 5e-5, -5e-5, 1.0 + 1e-3, 1e-5)


def synthetic_stacks(case, seed):
    """fp32 CPU stacks rgb [M,V,P,3], depth [M,V,P], acc [M,V,P], sem [S,V,P,C] of one case"""
    P, C, M, S, V, k = case
    gen = torch.Generator().manual_seed(seed)
    view = torch.arange(V) + seed                                        # alternates the regime view by view and, at V = 1, case by case
    # rgb: a common image plus member differences of std 0.05 (4000 x variance ~ 10 (M - 1) / M) or 0.4 (~ 640 (M - 1) / M: clipped at 100)
    rgb_std = torch.where(view % 2 == 0, 0.05, 0.4).view(1, V, 1, 1)
    rgb = torch.rand(1, V, P, 3, generator=gen) + rgb_std * torch.randn(M, V, P, 3, generator=gen)
    # depth: a large common offset plus small member differences (a one-pass sum-of-squares variance cancels here); every third view has
    # large differences (50 x variance ~ 450 (M - 1) / M: clipped)
    dep_std = torch.where(view % 3 == 1, 3.0, 1e-3).view(1, V, 1)
    depth = 5.0 + dep_std * torch.randn(M, V, P, generator=gen)
    acc = torch.rand(M, V, P, generator=gen)
    for j, x in enumerate(ACC_PLANTED):
        acc[:, :, (j + seed) % len(ACC_PLANTED)::len(ACC_PLANTED) + 1] = x
    if k >= 1e4:                                                         # about three classes at +1e4, the rest at -1e4: H ~ log(3)
        sem = torch.where(torch.rand(S, V, P, C, generator=gen) < 0.1, k, -k)
    else:
        sem = k * torch.randn(S, V, P, C, generator=gen)
    return rgb.float(), depth.float(), acc.float(), sem.float()


@pytest.fixture(scope="module")
def synthetic():
    """every case's stacks and the restatement's rows, computed once on the CPU and left unchanged"""
    out = []
    for i, case in enumerate(CASES):
        stacks = synthetic_stacks(case, i)
        out.append((stacks, ensemble_rows(*(s.numpy() for s in stacks)).T))
    return out


def test_synthetic_cases_reach_every_branch_of_the_restatement(synthetic):
    """What the golden does not exercise: both sides of every clip, in the restatement's own output."""
    rows = np.concatenate([want for _, want in synthetic])
    sem_rows = np.concatenate([want[:, 3] for (case, (_, want)) in zip(CASES, synthetic) if case[1] > 1])
    assert ((sem_rows > 0) & (sem_rows < 100)).any() and (sem_rows == 100.0).any()
    for (P, C, M, S, V, k), (_, want) in zip(CASES, synthetic):
        if k >= 1e4:
            assert np.isfinite(want).all() and ((want[:, 3] > 0) & (want[:, 3] < 100)).all()
        if M == 1:
            assert (want[:, :2] == 0).all()                              # a single member: variance exactly 0
    multi = np.concatenate([want for (case, (_, want)) in zip(CASES, synthetic) if case[2] > 1])
    for col in (0, 1):
        assert ((multi[:, col] > 0) & (multi[:, col] < 100)).any() and (multi[:, col] == 100.0).any()
    per_pixel = np.concatenate([1.0 / (st[2][0].double().numpy().reshape(-1) + 1e-4) - 1.0 for st, _ in synthetic])
    assert (per_pixel < 0).any() and (per_pixel > 10000).any()           # both per-pixel clip ends of column 2
    assert np.isfinite(rows).all()
    names = ("P", "C", "M", "S", "V", "k")                               # the list is a pairwise cover
    for a in range(6):
        for b in range(a + 1, 6):
            seen = {(c[a], c[b]) for c in CASES[:-1]}
            for x in {c[a] for c in CASES[:-1]}:
                for y in {c[b] for c in CASES[:-1]}:
                    assert (x, y) in seen or (names[a], names[b]) == ("M", "S") and y > x, (names[a], x, names[b], y)


@pytest.mark.parametrize("i", range(len(CASES)), ids=["P%d-C%d-M%d-S%d-V%d-k%g" % c for c in CASES])
def test_kernel_equals_restatement_on_synthetic_stacks(synthetic, i):
    stacks, want = synthetic[i]
    got = _terms(tuple(s.to(DEV) for s in stacks))
    print("max abs deviation per column", np.abs(got - want).max(0))
    np.testing.assert_allclose(got, want, **BAR)


# ------------------------------------------------------------------ 3. unaligned and non-contiguous inputs
@pytest.mark.parametrize("i", [CASES.index((65, 29, 2, 2, 3, 1e4)), CASES.index((1025, 64, 5, 1, 1, 1)), CASES.index((63, 33, 2, 1, 1, 1))])
def test_unaligned_and_strided_inputs_give_the_same_bits(synthetic, i):
    stacks = tuple(s.to(DEV) for s in synthetic[i][0])
    want = _terms(stacks)

    def shifted(t, by):                                                  # the same values, `by` floats into a larger buffer: 4-byte aligned only
        buf = torch.empty(t.numel() + 8, device=DEV)
        out = buf[by:by + t.numel()].view(t.shape)
        out.copy_(t)
        assert out.is_contiguous() and out.data_ptr() % 16 == 4 * by
        return out
    for by in (1, 2, 3):
        np.testing.assert_array_equal(_terms(tuple(shifted(t, by) for t in stacks)), want)
    rgb, depth, acc, sem = stacks
    strided = (rgb.permute(3, 0, 1, 2).contiguous().permute(1, 2, 3, 0), depth.transpose(1, 2).contiguous().transpose(1, 2), acc.double(),
               sem.transpose(2, 3).contiguous().transpose(2, 3))
    assert not strided[0].is_contiguous() and not strided[3].is_contiguous()
    np.testing.assert_array_equal(_terms(strided), want)


# ------------------------------------------------------------------ 4. batch independence and repeatability
def test_view_rows_do_not_depend_on_the_batch_and_repeat(golden):
    case = (1025, 29, 2, 1, 40, 1)                                       # five workgroups per view
    stacks = tuple(s.to(DEV) for s in synthetic_stacks(case, 3))
    g = golden("trajectory")
    for st in (stacks, tuple(_cu(a) for a in golden_stacks(g))):
        full = _terms(st)
        halves = [_terms(tuple(t[:, lo:hi] for t in st)) for lo, hi in ((0, 20), (20, 40))]
        np.testing.assert_array_equal(np.concatenate(halves), full)
        np.testing.assert_array_equal(_terms(tuple(t[:, 7:8] for t in st)), full[7:8])
        for _ in range(10):
            np.testing.assert_array_equal(_terms(st), full)


# ------------------------------------------------------------------ 5. / 6. the routes, and end to end against the golden
@pytest.fixture(scope="module")
def routes(golden):
    """the golden's fields and trajectory through every route, once"""
    from apnrf_amd import render as RD
    g = golden("trajectory")
    sc = scene_of(g)
    kw = sc["kw"]
    fields = [_hip_ngp_field(g, s) for s in g["param_seeds"]]
    ests = [_hip_estimator(sc), _hip_estimator(sc)]
    W, Hh, focal = (float(x) for x in g["whf"])
    args = (fields, ests, g["trajectory"], 1, int(W), int(Hh), focal, kw["near_plane"], kw["render_step_size"], kw["cone_angle"], kw["alpha_thre"])
    out = dict(one_call=RD.trajectory_uncertainty(*args, device=DEV), python=RD.trajectory_uncertainty(*args, device=DEV, one_call=False),
               no_group=RD.trajectory_uncertainty(*args, device=DEV, group=False),
               no_group_python=RD.trajectory_uncertainty(*args, device=DEV, group=False, one_call=False),
               last=RD.trajectory_uncertainty(*((args[:3]) + (-1,) + args[4:]), device=DEV))
    poses = g["trajectory"][RD.trajectory_view_indices(len(g["trajectory"]))]
    o, d, h, w = RD._pose_rays(poses, int(W), int(Hh), focal, 0.1, DEV)
    renders = [RD.render_views(f, e, o, d, h * w, 1024, near_plane=kw["near_plane"], render_step_size=kw["render_step_size"], render_bkgd=torch.zeros(3),
                               cone_angle=kw["cone_angle"], alpha_thre=kw["alpha_thre"]) for f, e in zip(fields, ests)]
    V = len(poses)
    out["views"] = RD.ensemble_view_terms(torch.stack([r["rgb"].view(V, h * w, 3) for r in renders]), torch.stack([r["depth"].view(V, h * w) for r in renders]),
                                          torch.stack([r["acc"].view(V, h * w) for r in renders]), renders[0]["sem"].view(V, h * w, -1)).cpu().numpy()
    return out


def test_routes_agree_bit_for_bit(routes, golden):
    g = golden("trajectory")
    unc, max_idx, rows = routes["one_call"]
    assert rows.shape == (4, 40) and rows.dtype == np.float64
    np.testing.assert_array_equal(max_idx, g["max_idx"])
    np.testing.assert_array_equal(rows.T, routes["views"])
    for k in ("python", "no_group", "no_group_python", "last"):
        np.testing.assert_array_equal(routes[k][2], rows, err_msg=k)
        np.testing.assert_array_equal(routes[k][1], max_idx)
    for k in ("python", "no_group", "no_group_python"):
        assert routes[k][0] == unc
    per_view = rows.sum(0)
    np.testing.assert_allclose(unc, per_view.mean(), rtol=1e-14)
    np.testing.assert_allclose(routes["last"][0], per_view[-11:].mean(), rtol=1e-14)


def test_end_to_end_rows_within_the_derived_bound_of_the_golden(routes, golden):
    """Poses -> rows against the reference's rows.  The renderer is held to 1e-3 absolute on rgb and acc and 1e-3 relative on depth
    (test_pose_drivers_equal_reference_dataset_golden); the 4000 x scale on a variance amplifies that, so the 5e-3 of `score_views` does
    not transfer.  With M = 2, var = ((a - b) / 2)^2: a per-render error eps moves a - b by at most 2 eps and the variance by at most
    |a - b| eps + eps^2.  Each row must lie inside TWICE the mean of that first-order bound over the golden's own stacks (acc: per pixel
    min(10000, eps / (acc + 1e-4)^2), the slope of 1 / (acc + 1e-4)); the semantic row is 100.0 in the golden and must be equal.
    Observed on the MI355X (deviation / bound, maximum over the 40 views): see DESIGN.md section 2."""
    g = golden("trajectory")
    rgb, depth, acc, _ = golden_stacks(g)
    eps = 1e-3
    bound_rgb = 4000.0 * (np.abs(rgb[0] - rgb[1]) * eps + eps ** 2).mean((1, 2))
    eps_d = eps * 0.5 * (np.abs(depth[0]) + np.abs(depth[1]))
    bound_dep = 50.0 * (np.abs(depth[0] - depth[1]) * eps_d + eps_d ** 2).mean(1)
    bound_acc = np.minimum(10000.0, eps / (acc[0] + 1e-4) ** 2).mean(1)
    rows = routes["one_call"][2]
    for k, (name, bound) in enumerate((("rgb", bound_rgb), ("depth", bound_dep), ("acc_inv", bound_acc))):
        dev = np.abs(rows[k] - g["rows"][k])
        print(f"{name}: max deviation {dev.max():.4g}, max bound {bound.max():.4g}, max deviation / bound {(dev / bound).max():.4g}")
        assert (dev <= 2 * bound).all(), (name, dev.max(), (dev / bound).max())
    np.testing.assert_array_equal(rows[3], g["rows"][3])
    assert (rows[3] == 100.0).all()
    for key, k in (("unc_step1", "one_call"), ("unc_stepm1", "last")):
        print(f"{key}: {routes[k][0]:.6f} against the reference's {float(g[key]):.6f}")


# ------------------------------------------------------------------ 7. error handling
def test_bad_sizes_return_the_error_code_and_launch_nothing():
    from apnrf_amd import _lib as L
    from apnrf_amd import render as RD
    lib = L.load_library()
    V, P = 2, 5
    terms = torch.full((V, 4), -7.0, dtype=torch.float64, device=DEV)
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device=DEV)

    def call(M, S, C):
        n = max(M, 1)
        rgb, dep, acc = torch.rand(n, V, P, 3, device=DEV), torch.rand(n, V, P, device=DEV), torch.rand(n, V, P, device=DEV)
        sem = torch.rand(max(S, 1), V, P, C, device=DEV)
        return lib.mnf_score_ensemble_views(rgb.data_ptr(), dep.data_ptr(), acc.data_ptr(), sem.data_ptr(), M, S, V, P, C, terms.data_ptr(), ws.data_ptr(),
                                            ws.numel(), L.stream())
    MNF_ERR_INVALID, MNF_ERR_UNSUPPORTED = -1, -3
    assert call(0, 1, 4) == MNF_ERR_INVALID and b"n_members" in lib.mnf_last_error()
    assert call(2, 3, 4) == MNF_ERR_INVALID and b"n_sem_members" in lib.mnf_last_error()
    assert call(2, 0, 4) == MNF_ERR_INVALID
    assert call(RD.ENSEMBLE_MAX_MEMBERS + 1, 1, 4) == MNF_ERR_UNSUPPORTED
    assert call(2, 1, RD.ENSEMBLE_MAX_CLASSES + 1) == MNF_ERR_UNSUPPORTED and b"supported" in lib.mnf_last_error()
    assert lib.mnf_score_ensemble_views_workspace_bytes(V, P, RD.ENSEMBLE_MAX_CLASSES + 1) == 0
    torch.cuda.synchronize()
    assert (terms == -7.0).all()                                         # nothing was launched
    assert call(RD.ENSEMBLE_MAX_MEMBERS, 2, 4) == 0                      # the maxima themselves are served
    torch.cuda.synchronize()
    assert torch.isfinite(terms).all() and (terms != -7.0).all()
    r = lambda *s: torch.rand(*s, device=DEV)
    for M, S, C in ((0, 1, 4), (2, 3, 4), (RD.ENSEMBLE_MAX_MEMBERS + 1, 1, 4), (2, 1, RD.ENSEMBLE_MAX_CLASSES + 1)):
        with pytest.raises(L.MnfError):
            RD.ensemble_view_terms(r(M, V, P, 3), r(M, V, P), r(M, V, P), r(S, V, P, C))
    with pytest.raises(ValueError):
        RD.ensemble_view_terms(r(2, V, P, 3), r(2, V, P + 1), r(2, V, P), r(1, V, P, 4))
    with pytest.raises(L.MnfError):
        RD.ensemble_view_terms(r(2, V, P, 3).cpu(), r(2, V, P), r(2, V, P), r(1, V, P, 4))


# ------------------------------------------------------------------ 8. the scoring workspace at exactly its size (csrc/score.hip: carve_score)
SENTINEL, TAIL = 0xA5, 4096


@pytest.fixture(scope="module")
def ensemble(golden):
    g = golden("trajectory")
    sc = scene_of(g)
    return g, sc["kw"], [_hip_ngp_field(g, s) for s in g["param_seeds"]], [_hip_estimator(sc), _hip_estimator(sc)]


# members x views: two groups of 1 and 2 views per member, three groups of one view, four uneven groups (1, 1, 1, 2 views)
@pytest.mark.parametrize("M,V", [(2, 3), (1, 3), (1, 5)])
@pytest.mark.parametrize("name", ["mnf_score_poses", "mnf_score_trajectory"])
def test_scoring_fits_exactly_the_workspace_it_asks_for(ensemble, name, M, V):
    """Both one-call scorers, through `_lib` directly, in a workspace of exactly the size their size function returns, with a sentinel
    tail behind it: the terms are those of the same call in a workspace 1 MB larger, no byte behind the size is written, and one
    byte less is refused.  The size is the layout run on a null base, so nothing pads it: the tail is what shows that it suffices."""
    import ctypes
    from apnrf_amd import _lib as L
    from apnrf_amd import render as RD
    g, kw, fields, ests = ensemble
    lib = L.load_library()
    W, Hh, focal = (float(x) for x in g["whf"])
    W, Hh, P = int(W), int(Hh), 8 * 8
    poses = np.asarray(g["trajectory"])[RD.trajectory_view_indices(len(g["trajectory"]))][:V]
    c2w = torch.from_numpy(np.stack([RD.pose_to_c2w(np.asarray(p, np.float64)) for p in poses]).astype(np.float32)[:, :3, :4].copy()).to(DEV)
    idx = torch.from_numpy(RD.subsample_indices(W * Hh, P)).to(DEV)
    handles = (ctypes.c_void_p * M)(*[f._ensure_handle() for f in fields[:M]])
    grids = [RD._grid_args(e) for e in ests[:M]]
    bins = (ctypes.c_void_p * M)(*[x.binaries.data_ptr() for x in grids])
    bits = (ctypes.c_void_p * M)(*[x.bits.data_ptr() for x in grids])
    ropts = RD._render_opts(max_samples=1024, far_plane=1e10, early_stop_eps=1e-4, rays_per_view=P, n_levels=grids[0].n_levels, near_plane=kw["near_plane"],
                            render_step_size=kw["render_step_size"], cone_angle=kw["cone_angle"], alpha_thre=kw["alpha_thre"],
                            probabilistic=name == "mnf_score_poses")
    nbytes = int(getattr(lib, name + "_workspace_bytes")(M, V, P, fields[0].num_semantic_classes))
    assert nbytes > 0

    def run(ws, given):
        terms = torch.full((V, 4), float("nan"), dtype=torch.float64, device=DEV)
        L.launch(getattr(lib, name), handles, bins, bits, M, *grids[0].res, grids[0].aabb, L.ptr(c2w), V, W, Hh, float(np.float32(focal)), L.ptr(idx), P,
                 ctypes.byref(ropts), L.ptr(terms), L.ptr(ws), given)
        torch.cuda.synchronize()
        return terms

    roomy = run(torch.zeros(nbytes + (1 << 20), dtype=torch.uint8, device=DEV), nbytes + (1 << 20))
    exact_ws = torch.full((nbytes + TAIL,), SENTINEL, dtype=torch.uint8, device=DEV)
    exact = run(exact_ws, nbytes)
    assert torch.isfinite(roomy).all()
    assert torch.equal(exact, roomy)
    assert bool((exact_ws[nbytes:] == SENTINEL).all()), "a byte behind the size the library asked for was written"
    with pytest.raises(L.MnfError, match="workspace too small"):
        run(exact_ws, nbytes - 1)
