"""GPU tests of the fused test renderers (`mnf_render_jobs` behind `render.render_views` / `render_image_with_occgrid_test`) away from the yaml's four
render options (`scenes.RENDER_KW`): the reference functions' own defaults (cone angle 0: round budgets of 1, 2 and 3 samples, 64 / 32 / 21 rays per tile,
runs across lane 31 / 32 of the general compositing path; alpha threshold 0: every valid sample kept), `early_stop_eps` other than 1e-4, a near plane beyond
the first surfaces and a far plane inside the box, a threshold that leaves whole tiles dead, and sample budgets that end a render while rays are alive.

Reference: `oracle.render.render_prob_test` (the deterministic renderer's outputs are the same loop without the two variances: one oracle render serves
both), pinned to the running reference at these options by tests/test_render_options_golden_cpu.py.

Every case carries two conditions of its own, asserted before the GPU is compared with anything:
  * the oracle's record shows that the case reaches the path it is here for (`_REACHES`);
  * the oracle rendered a second time with its matrix products added up in another order (`accum="k16_reversed"`) has the same round schedule, the same
    kept and marched totals and no ray further than 1e-3 away: the case's answer does not hang on an fp32 rounding, so the GPU has no excuse.
Bars: rgb, acc, depth, rgb_var, depth_var 1e-3 absolute; class logits max(1e-3, 3e-4 x the ray's largest |logit|).  STRICT cases (the
schedule depends on geometry alone, or on nothing a rounding moves): no ray outside the bars, kept and marched totals exact.  The others: at most 2 rays
outside (an alpha-threshold or opacity tie), none beyond 5e-2, kept total within 2, marched total exact."""
import functools

import numpy as np
import pytest
import torch

import helpers as H

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BK = torch.tensor([0.1, 0.3, 0.6])
DEFAULTS = dict(near_plane=0.0, far_plane=1e10, render_step_size=5e-3, cone_angle=0.0, alpha_thre=0.0, early_stop_eps=1e-4)      # utils.py:555-569 (step coarsened)

# id -> (render options, max_samples, strict, background)
CASES = {
    "R1": (DEFAULTS, 1024, True, BK),
    "R2": (dict(near_plane=0.05, render_step_size=4e-3, cone_angle=0.0, alpha_thre=0.0, early_stop_eps=0.0), 200, True, BK),
    "R3": (dict(near_plane=0.1, render_step_size=2e-3, cone_angle=0.004, alpha_thre=0.0, early_stop_eps=0.2), 1024, False, BK),
    "R4": (dict(near_plane=0.8, far_plane=3.0, render_step_size=2e-3, cone_angle=0.01, alpha_thre=0.05), 1024, False, BK),
    "R5": (dict(near_plane=0.1, render_step_size=2e-2, cone_angle=0.004, alpha_thre=0.3), 1024, False, torch.zeros(3)),
    "R6": (H.RENDER_KW, 50, False, BK),
    # R7 is R1's options with early_stop_eps 0.05 in place of 1e-4.  At 1e-4 the render missed on the MI355X by one ray's last round (kept and marched 36 632 against
    # 36 635, every value inside the bars): ray 555 has, after the stride-3 round 74, an opacity of EXACTLY fp32(1 - 1e-4) in both oracle runs, so `opacity <= opc_thre`
    # (utils.py:751) hangs on the last bit of a sum which the kernel adds up in another order (a round's weights first, then the ray's opacity) than index_add_ does.  Near
    # 0.9999 a sample adds ~1e-5 and an fp32 ulp is 6e-8, so with 576 rays such ties cannot be chosen away at that eps (`opacity_gap` below: 0 to 3e-7 for every pose and step
    # tried); at 0.05 the closest ray stays 4.7e-6 (80 ulp) away and the strides 1, 2, 3 are still there.
    "R7": (dict(DEFAULTS, early_stop_eps=0.05), 1024, True, BK),
    # R9 (not in the issue's table): what tells `alpha >= alpha_thre` from `alpha > alpha_thre` (utils.py:714).  A sample ON the threshold cannot be aimed at through
    # the MLP, but fp32 has one alpha that many samples share to the bit: 1 - exp(-sigma dt) == 1.0f once sigma dt > 17.4.  The density row of the base MLP is scaled
    # by 2, the threshold is 1.0: the reference keeps exactly the saturated samples (2 374 of 8 387 marched), `>` keeps none.
    "R9": (dict(near_plane=0.1, render_step_size=2e-2, cone_angle=0.004, alpha_thre=1.0), 1024, False, BK),
    "R8": (dict(DEFAULTS, render_step_size=2e-2), 1024, True, BK),      # (step 2e-2: 51 and 67 rounds in place of 195 and 261 at 5e-3, whose four oracle renders of the 64 x 4 field take 25 s)
}
# Strict cases whose schedule depends on opacities: no ray that could go on may come closer than this to the other side of the retirement test `opacity <= opc_thre`
# in either oracle run (`opacity_gap`).  1e-6 is 16 fp32 ulp of an opacity near 1: adding a round's <= 64 weights in another order moves the sum by a few ulp, the
# oracle's own two accumulation orders by one or two.  R1 (and R2, whose threshold is 1.0) keep the numbers the reference functions default to, at which the gap is 0 (see R7):
# they are exact on the MI355X today, and a miss by one ray's round there would be this tie.
MIN_OPACITY_GAP = {"R7": 1e-6, "R8": 1e-6}
RPV = 576      # 24 x 24 rays per view: neither a multiple of 64 nor of the march workgroup's 1024 threads


def _strides(ref):
    return {s for _, s in ref["rounds"]}


# what the oracle's own record must show for the case to be the case
_REACHES = {
    "R1": lambda ref, bk: {1, 2, 3} <= _strides(ref),
    "R2": lambda ref, bk: ref["alive_at_end"] > 0 and sum(s for _, s in ref["rounds"]) >= 200,
    "R3": lambda ref, bk: 0.5 < float(ref["acc"].mean()) < 0.95,
    "R4": lambda ref, bk: int(((ref["acc"][:, 0] == 0) & (ref["rgb"] == bk).all(1)).sum()) >= 0.1 * RPV,
    "R5": lambda ref, bk: 0 < ref["total_samples"] < 0.5 * ref["marched_samples"],
    "R6": lambda ref, bk: sum(s for _, s in ref["rounds"]) == 52,
    "R7": lambda ref, bk: {1, 2, 3} <= _strides(ref),
    "R8": lambda ref, bk: {1, 2, 3} <= _strides(ref),
    "R9": lambda ref, bk: 500 <= ref["total_samples"] < 0.5 * ref["marched_samples"] and float(ref["acc"].mean()) > 0.3,
}


def _two_level_scene():
    """The two-level estimator and field of glue_ngp.npz's `ml_*` case, as tests/test_gpu_round5.py builds them; (field scene, occ, aabbs, roi)"""
    import os
    from apnrf_amd import synthetic as S
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "glue_ngp.npz"))
    occ = np.unpackbits(g["ml_occ"])[: 2 * 50 * 12 * 50].reshape(2, 50, 12, 50).astype(bool)
    aabbs, lh = g["ml_aabbs"], int(g["log2_hashmap_size"])
    scene = dict(aabb=aabbs[-1].astype(np.float32), neurons=128, layers=2, C=29, log2_hashmap_size=lh,
                 params=S.make_field_params(128, 2, 29, seed=int(g["param_seed"]), log2_hashmap_size=lh))
    return scene, occ, aabbs, g["ml_roi"]


def _inputs(case):
    """-> dict(sc [the field's scene], occ, aabbs, roi | None, views [list of (o, d)])"""
    if case == "R7":
        fs, occ, aabbs, roi = _two_level_scene()
        o, d = H.view_rays(H.make_scene(log2_hashmap_size=12), 3, h=24, w=24)      # (the poses only: as make_golden's `_view(sc, 3, ...)`)
        return dict(sc=fs, occ=occ, aabbs=aabbs, roi=roi, views=[(o + torch.tensor([3.0, 0.0, 3.0]), d)])      # inside the roi
    if case == "R8":
        sc = H.make_scene(neurons=64, layers=4, C=13, log2_hashmap_size=14, seed=2)
        views = [H.view_rays(sc, 1, h=24, w=24), H.view_rays(sc, 6, h=24, w=24)]
    else:
        sc = H.make_scene(log2_hashmap_size=14, seed=2)
        if case == "R9":
            from test_gpu_tile_skip import scale_density_row
            scale_density_row(sc, 2.0)
        views = [H.view_rays(sc, 1, h=24, w=24)]
    return dict(sc=sc, occ=sc["occ"], aabbs=None, roi=None, views=views)


def _oracle_render(inp, kw, max_samples, bk, accum):
    """One oracle render per view (the reference function renders one view per call)"""
    from oracle import render as R
    orc = H.oracle_field(inp["sc"], accum=accum)
    outs = []
    for o, d in inp["views"]:
        aabbs = inp["aabbs"] if inp["aabbs"] is not None else inp["est_aabbs"]
        outs.append(R.render_prob_test(max_samples, orc, inp["occ"], aabbs, o, d, render_bkgd=bk, **kw))
    return outs


@functools.lru_cache(maxsize=None)
def oracle_case(case):
    """The case's inputs and its oracle renders under both accumulation orders, computed once and shared by the case's tests (never written to).  Needs no GPU:
    the estimator's box is taken from a CPU estimator (`aabbs[0]` is the scene box re-derived from centre and extent, occ_grid.py, and can differ from it in the
    last bits)."""
    from apnrf_amd.nerfacc import OccGridEstimator
    kw, max_samples, strict, bk = CASES[case]
    inp = _inputs(case)
    if inp["aabbs"] is None:
        inp["est_aabbs"] = OccGridEstimator(torch.from_numpy(inp["sc"]["aabb"]), resolution=inp["sc"]["res"], levels=1).aabbs.numpy()
    refs = _oracle_render(inp, kw, max_samples, bk, "whole")
    again = _oracle_render(inp, kw, max_samples, bk, "k16_reversed")
    return inp, refs, again


def check_case_is_valid(case, verbose=True):
    """The two conditions of the module docstring, on the CPU.  A case that fails here is not a valid input and is changed, never given a wider budget."""
    kw, max_samples, strict, bk = CASES[case]
    inp, refs, again = oracle_case(case)
    for v, (a, b) in enumerate(zip(refs, again)):
        assert a["rounds"] == b["rounds"], (case, v, "the round schedule depends on the accumulation order")
        assert (a["total_samples"], a["marched_samples"]) == (b["total_samples"], b["marched_samples"]), (case, v, a["total_samples"], b["total_samples"])
        worst = max(float((a[k] - b[k]).abs().max()) for k in ("rgb", "acc", "depth", "sem", "rgb_var", "depth_var"))
        if verbose:
            print(f"{case} view {v}: {len(a['rounds'])} rounds, strides {sorted(_strides(a))}, kept {a['total_samples']} of {a['marched_samples']} marched, "
                  f"mean acc {float(a['acc'].mean()):.3f}, empty rays {int((a['acc'] == 0).sum())}, oracle against itself {worst:.2e}, "
                  f"opacity gap {a['opacity_gap']:.2e}")
        assert worst <= 1e-3, (case, v, worst)
        assert _REACHES[case](a, bk), (case, v, "the case no longer reaches its path")
        if case in MIN_OPACITY_GAP:
            assert min(a["opacity_gap"], b["opacity_gap"]) >= MIN_OPACITY_GAP[case], (case, v, a["opacity_gap"], b["opacity_gap"])
    if case == "R8":
        assert refs[0]["rounds"] != refs[1]["rounds"], "the two views of R8 must have different schedules"


def _estimator(inp):
    if inp["roi"] is None:
        return H.hip_estimator(inp["sc"])
    from apnrf_amd.nerfacc import OccGridEstimator
    est = OccGridEstimator(torch.from_numpy(inp["roi"]), resolution=[50, 12, 50], levels=2)
    est.binaries = torch.from_numpy(inp["occ"])
    est = est.to(DEV).eval()
    np.testing.assert_array_equal(est.aabbs.cpu().numpy(), inp["aabbs"])
    return est


def _compare(case, prob, out, refs, n_views):
    """The module docstring's bars, view by view; prints every figure before it asserts."""
    strict = CASES[case][2]
    keys = ("rgb", "acc", "depth", "sem") + (("rgb_var", "depth_var") if prob else ())
    kept = marched = 0
    for v in range(n_views):
        ref = refs[v]
        sl = slice(v * RPV, (v + 1) * RPV)
        bad = np.zeros(RPV, bool)
        worst = {}
        for k in keys:
            got, want = out[k][sl].cpu().numpy().reshape(RPV, -1), ref[k].numpy().reshape(RPV, -1)
            assert np.isfinite(got).all(), (case, k)
            bar = np.maximum(1e-3, 3e-4 * np.abs(want).max(1, keepdims=True)) if k == "sem" else 1e-3
            err = np.abs(got - want)
            worst[k] = float(err.max())
            bad |= (err > bar).any(1)
            assert err.max() <= (np.max(bar) if strict else 5e-2), (case, v, k, float(err.max()))
        print(f"{case} prob={prob} view {v}: " + ", ".join(f"{k} {e:.2e}" for k, e in worst.items()) + f"; rays outside the bars {int(bad.sum())}")
        assert bad.sum() <= (0 if strict else 2), (case, v, int(bad.sum()))
        kept += ref["total_samples"]; marched += ref["marched_samples"]
    got_kept, got_marched = int(out["total"][0]), int(out["total"][1])
    print(f"{case} prob={prob}: kept {got_kept} vs oracle {kept}, marched {got_marched} vs oracle {marched}")
    assert abs(got_kept - kept) <= (0 if strict else 2), (case, got_kept, kept)
    assert got_marched == marched, (case, got_marched, marched)


@pytest.mark.parametrize("prob", [False, True])
@pytest.mark.parametrize("case", list(CASES))
def test_fused_renderer_at_options(case, prob):
    from apnrf_amd import render as RD
    check_case_is_valid(case)
    kw, max_samples, strict, bk = CASES[case]
    inp, refs, _ = oracle_case(case)
    hip, est = H.hip_field(inp["sc"]), _estimator(inp)
    if inp["roi"] is None:
        np.testing.assert_array_equal(est.aabbs.cpu().numpy(), inp["est_aabbs"])
    V = len(inp["views"])
    o = torch.cat([o_ for o_, _ in inp["views"]]).to(DEV)
    d = torch.cat([d_ for _, d_ in inp["views"]]).to(DEV)
    # (n_split=1: the views of one call are ONE render job, their budgets side by side in every launch)
    out = RD.render_views(hip, est, o, d, RPV, max_samples, render_bkgd=bk, probabilistic=prob, n_split=1, **kw)
    _compare(case, prob, out, refs, V)
    if case == "R1":
        # the reference's own signature with its own defaults (near 0, far 1e10, cone 0, alpha_thre 0, eps 1e-4): the same render, bit for bit
        rays = RD.Rays(o, d)
        if prob:
            rgb, rgb_var, acc, depth, depth_var, sem, tot = RD.render_probablistic_image_with_occgrid_test(1024, hip, est, rays, render_step_size=5e-3, render_bkgd=bk)
            assert torch.equal(rgb_var, out["rgb_var"]) and torch.equal(depth_var, out["depth_var"])
        else:
            rgb, acc, depth, sem, tot = RD.render_image_with_occgrid_test(1024, hip, est, rays, render_step_size=5e-3, render_bkgd=bk)
        assert torch.equal(rgb, out["rgb"]) and torch.equal(acc, out["acc"]) and torch.equal(depth, out["depth"]) and torch.equal(sem, out["sem"])
        assert tot == int(out["total"][0]) == refs[0]["total_samples"]
    if case == "R8":
        # batch independence at strides 1 to 3: each view of the two-view call equals the same view rendered alone, bit for bit, and so does the call cut
        # into two jobs (n_split=2, the default)
        split = RD.render_views(hip, est, o, d, RPV, max_samples, render_bkgd=bk, probabilistic=prob, **kw)
        kept = 0
        for v in range(V):
            sl = slice(v * RPV, (v + 1) * RPV)
            alone = RD.render_views(hip, est, o[sl], d[sl], RPV, max_samples, render_bkgd=bk, probabilistic=prob, **kw)
            kept += int(alone["total"][0])
            assert int(alone["total"][0]) == refs[v]["total_samples"] and int(alone["total"][1]) == refs[v]["marched_samples"]
            for k in alone:
                if k != "total":
                    assert torch.equal(alone[k], out[k][sl]), (k, v)
                    assert torch.equal(alone[k], split[k][sl]), (k, v, "two jobs")
        assert kept == int(out["total"][0]) == int(split["total"][0])
