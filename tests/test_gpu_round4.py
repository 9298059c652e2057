"""Round-4 GPU tests: the one-call train step against the oracle's autograd; the reference's
dynamic ray-count schedule (scripts/pipeline.py:494-504) through the asynchronous train step; full-size checks of BASELINE configs 3 and 4."""
import numpy as np
import pytest
import torch

import helpers as H

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _rel(a, b):
    return float((a - b).norm() / (b.norm() + 1e-30))


def test_train_step_c_call_is_repeatable_and_matches_oracle_autograd():
    """The whole train step as one C call (`mnf_train_step`): two runs agree within float-atomics noise (same sample counts and losses), and the
    gradients sit within the fp16 gradient tolerance of the oracle's autograd."""
    from apnrf_amd import render as RD
    from oracle import render as R
    sc = H.make_scene(log2_hashmap_size=15)
    o, d = H.view_rays(sc, 2, h=20, w=20)
    rng = np.random.default_rng(3)
    n = o.shape[0]
    pix = torch.from_numpy(rng.random((n, 3)).astype(np.float32)); dep = torch.from_numpy(rng.uniform(0.5, 4.0, n).astype(np.float32))
    lab = torch.from_numpy(rng.integers(0, sc["C"], n))
    bk = torch.tensor([0.1, 0.5, 0.9])
    res = {}
    for mode in (1, 2):
        hip, est = H.hip_field(sc).train(), H.hip_estimator(sc)
        out = RD.fused_forward_backward(hip, est, RD.Rays(o.to(DEV), d.to(DEV)), pix.to(DEV), dep.to(DEV), lab.to(DEV), bk.to(DEV), stratified=False, **H.RENDER_KW)
        res[mode] = (out["n_rendering_samples"], float(out["loss"]), [p.grad.clone() for p in (hip.mlp_base.params, hip.mlp_head.params, hip.mlp_sem.params)])
    assert res[1][0] == res[2][0] and res[1][0] > 2000
    assert abs(res[1][1] - res[2][1]) <= 1e-6 * abs(res[1][1])
    for a, b in zip(res[2][2], res[1][2]):
        assert _rel(a, b) < 1e-5
    # oracle autograd on the same batch
    import torch.nn.functional as F
    orc = H.oracle_field(sc, "f16", requires_grad=True)
    est = H.hip_estimator(sc)
    ref = R.render_train(orc, sc["occ"], sc["aabb"][None], float(est.occs.mean().item()), o, d, torch.full((n,), 0.1), render_bkgd=bk,
                         render_step_size=1e-3, cone_angle=0.004, alpha_thre=0.01)
    loss = F.smooth_l1_loss(ref[0], pix) * 10 + F.smooth_l1_loss(ref[2], dep.unsqueeze(1)) / 5 + F.cross_entropy(ref[3], lab) / 2
    loss.backward()
    assert ref[4] == res[2][0]
    assert abs(float(loss.detach()) - res[2][1]) < 5e-4 * max(1.0, abs(float(loss.detach())))
    for got, want in zip(res[2][2], (orc.p_base.grad, orc.p_head.grad, orc.p_sem.grad)):
        w = want.to(DEV)
        assert _rel(got, w) < 5e-2 and torch.nn.functional.cosine_similarity(got, w, dim=0) > 0.998, (_rel(got, w),)


def test_dynamic_ray_count_schedule_async_matches_sync():
    """scripts/pipeline.py:494-504: `num_rays` is recomputed after EVERY iteration (capped at 2000) to hold the sample count near the target.
    The asynchronous train step keeps ONE state per field whatever the ray count: replaying the synchronous run's ray
    counts without any host round trip gives the same trajectory (float-atomics noise), one train state, a bounded pool of pinned buffers,
    and a flagged step (bad class id) still surfaces although every step has a different ray count."""
    from apnrf_amd import _lib as L
    from apnrf_amd import render as RD
    from apnrf_amd.optim import FusedAdam
    sc = H.make_scene(log2_hashmap_size=15)
    o_all, d_all = H.view_rays(sc, 1, h=64, w=64)
    rng = np.random.default_rng(11)
    pix_all = torch.from_numpy(rng.random((4096, 3)).astype(np.float32)); dep_all = torch.from_numpy(rng.uniform(0.5, 4.0, 4096).astype(np.float32))
    lab_all = torch.from_numpy(rng.integers(0, sc["C"], 4096))
    perms = [torch.from_numpy(np.random.default_rng(100 + k).permutation(4096)) for k in range(40)]
    target, bk = 1 << 15, torch.tensor([0.2, 0.2, 0.2], device=DEV)

    def run(sync, schedule=None):
        torch.manual_seed(77)                                          # the occupancy refresh draws its device seeds from torch's generator
        hip, est = H.hip_field(sc).train(), H.hip_estimator(sc)
        if not sync:
            RD.reserve_sample_bounds(hip, 3 << 20, 1 << 20)             # (this random-init scene marches ~900 samples per ray: beyond the per-ray defaults)
        opt = FusedAdam(hip.parameters(), lr=1e-3, eps=1e-15).bind_field(hip)
        R_, rs, losses, skipped = 1024, [], [], 0
        for k in range(40):
            R_ = schedule[k] if schedule is not None else R_
            sel = perms[k][:R_]
            out = RD.train_step(hip, est, opt, RD.Rays(o_all[sel].to(DEV), d_all[sel].to(DEV)), pix_all[sel].to(DEV), dep_all[sel].to(DEV),
                                lab_all[sel].to(DEV), bk, step=k + 1, sync=sync, stratified=False, **H.RENDER_KW)
            rs.append(R_); losses.append(out["loss"]); skipped += int(out["skipped"]) if sync else 0
            if schedule is None:
                n = out["n_rendering_samples"]
                R_ = min(2000, max(16, int(R_ * target / n)))           # pipeline.py:494-504 (update_num_rays(min(2000, num_rays)))
        return hip, rs, [float(x) for x in losses], skipped
    _, rs, loss_sync, skipped = run(True)
    assert skipped == 0 and len(set(rs)) > 10, rs                       # the ray count really changes from step to step (overflowing steps were repeated)
    n_states = len(RD._TRAIN_STATE)
    hip, rs2, loss_async, _ = run(False, rs)
    assert len(RD._TRAIN_STATE) <= n_states + 1                          # one more field, ONE state for its 40 different ray counts
    st = RD._TRAIN_STATE[id(hip)]
    assert len(st.pending) + len(st.pinned) <= 4 and st.overflowed_steps == 0
    assert RD.latest_step_counts(hip) is not None and RD.latest_step_counts(hip)[0] in rs
    np.testing.assert_allclose(loss_async, loss_sync, rtol=5e-3)
    # a flagged step among changing ray counts is not lost: the error surfaces within the next two calls
    bad = lab_all.clone(); bad[:] = sc["C"] + 3
    opt = FusedAdam(hip.parameters(), lr=1e-3, eps=1e-15).bind_field(hip)
    with pytest.raises(L.MnfError, match="class id"):
        for k, R_ in enumerate((300, 411, 522, 633)):
            sel = perms[k][:R_]
            RD.train_step(hip, H.hip_estimator(sc), opt, RD.Rays(o_all[sel].to(DEV), d_all[sel].to(DEV)), pix_all[sel].to(DEV), dep_all[sel].to(DEV),
                          (bad if k == 0 else lab_all)[sel].to(DEV), bk, step=100 + k, sync=False, stratified=False, **H.RENDER_KW)
        torch.cuda.synchronize()
        RD.train_step(hip, H.hip_estimator(sc), opt, RD.Rays(o_all[:64].to(DEV), d_all[:64].to(DEV)), pix_all[:64].to(DEV), dep_all[:64].to(DEV), lab_all[:64].to(DEV), bk,
                      step=200, sync=False, stratified=False, **H.RENDER_KW)


# ------------------------------------------------------------------ BASELINE configs 3 and 4 at the benchmark's own size, trained weights
def _render_errors(got, ref, n):
    """per-ray max |error| of rgb / acc / depth / composited class logits; the logits both ways: absolute (the north star's 1e-3) and relative to
    max(1, largest |logit| of the ray) (on trained weights the logits reach +-50 and carry fp16's relative error)."""
    errs = {k: (got[k].cpu() - ref[k]).abs().reshape(n, -1).max(dim=1).values.numpy() for k in ("rgb", "acc", "depth", "sem")}
    sem_mag = np.maximum(1.0, ref["sem"].abs().max(dim=1).values.numpy())
    # bar for the logits: max(1e-3, 3e-4 x |logit|) = 3x the oracle's own accumulation-order noise floor (tests/test_oracle_noise_floor_cpu.py;
    # measured on THIS scene below)
    return errs, errs["sem"] / np.maximum(1.0, 0.3 * sem_mag), sem_mag


def test_config3_trained_scene_sparse_parity_at_1e3():
    """BASELINE config 3 as bench.py renders it: the 2000-iteration stand-in of scene 102344529, an 800x800 view, a 24x24
    linspace sub-sample of its rays rendered stand-alone on the GPU and through the oracle (same call shape, hence the same round schedule):
    rgb / acc / depth within 1e-3 absolute, class logits within 1e-3 x max(1, |logit|) — both forms reported — with the tie budget (<= 2 rays up
    to 5e-2: a sample on the alpha-threshold edge), PSNR > 50 dB, evaluated-sample totals within 0.2 %.
    The same checks run a second time with the trained state in the tcnn-faithful mode (`tcnn_output_rounding=True`: every network output handed
    over in fp16) against the oracle's precision="tcnn", its noise floor taken from the "tcnn" oracle with permuted accumulation."""
    from apnrf_amd import render as RD
    from apnrf_amd import standin as SI
    from oracle import render as R
    sc = H.make_scene("102344529", n_poses=40)
    field, est, _ = SI.train_standin(sc, DEV, steps=2000, seed=9)
    from oracle.field import FieldConfig, OracleField
    cfg = FieldConfig(aabb=tuple(float(x) for x in sc["aabb"]), neurons=sc["neurons"], layers=sc["layers"], num_semantic_classes=sc["C"],
                      log2_hashmap_size=sc["log2_hashmap_size"])
    params = {"mlp_base": field.mlp_base.params.detach().cpu().numpy(), "mlp_head": field.mlp_head.params.detach().cpu().numpy(),
              "mlp_sem": field.mlp_sem.params.detach().cpu().numpy()}
    field_tcnn = H.hip_field(dict(sc, params=params), tcnn_output_rounding=True)       # the same trained state, fp16 hand-over
    occ = est.binaries.cpu().numpy()
    S_, width = 24, 800
    focal = 0.5 * width / np.tan(np.pi / 4)
    bk = torch.zeros(3)
    worst_all = []
    for mode, hip, prec in (("f16", field, "f16"), ("tcnn", field_tcnn, "tcnn")):
        orc = OracleField(cfg, params, prec, False)
        orc_perm = OracleField(cfg, params, prec, False, accum="k16_reversed")     # same operands, another fp32 accumulation order: the noise floor
        outs = []
        for pose in (0, 15):
            idx = R.subsample_indices(width * width, S_ * S_)
            o, d = R.generate_image_rays(R.pose_to_c2w(sc["poses"][pose]), width, width, focal, idx)
            ref = R.render_test(1024, orc, occ, sc["aabb"][None], o, d, render_bkgd=bk, **H.RENDER_KW)
            got = RD.render_views(hip, est, o.to(DEV), d.to(DEV), S_ * S_, 1024, render_bkgd=bk, **H.RENDER_KW)
            outs.append(got["sem"])
            errs, sem_scaled, sem_mag = _render_errors(got, ref, S_ * S_)
            ref2 = R.render_test(1024, orc_perm, occ, sc["aabb"][None], o, d, render_bkgd=bk, **H.RENDER_KW)
            floor = (ref2["sem"] - ref["sem"]).abs().max(dim=1).values.numpy()
            print(f"config 3 [{mode}] pose {pose}: NOISE FLOOR of the composited logits (oracle vs oracle, permuted accumulation): abs {floor.max():.2e} "
                  f"({int((floor > 1e-3).sum())} rays above 1e-3), relative to the ray's largest |logit| {(floor / sem_mag).max():.2e}; "
                  f"HIP vs oracle: abs {errs['sem'].max():.2e}, relative {(errs['sem'] / sem_mag).max():.2e}")
            assert (errs["sem"] / sem_mag).max() <= 3.0 * max((floor / sem_mag).max(), 1e-4)      # the product sits within 3x the oracle's own floor
            worst = np.max(np.stack([errs["rgb"], errs["acc"], errs["depth"], sem_scaled]), axis=0)
            tie = worst > 1e-3
            mse = float(((got["rgb"].cpu() - ref["rgb"]) ** 2).mean())
            print(f"config 3 [{mode}] pose {pose}: max abs rgb {errs['rgb'][~tie].max():.2e} acc {errs['acc'][~tie].max():.2e} depth {errs['depth'][~tie].max():.2e} | "
                  f"sem scaled {sem_scaled[~tie].max():.2e}, unscaled {errs['sem'].max():.2e} ({int((errs['sem'] > 1e-3).sum())} rays above 1e-3 absolute, "
                  f"largest |logit| {sem_mag.max():.1f}) | tie rays {int(tie.sum())} | PSNR {10 * np.log10(1.0 / max(mse, 1e-20)):.1f} dB | "
                  f"samples {int(got['total'][0])} vs {ref['total_samples']}")
            assert worst[~tie].max() <= 1e-3 and tie.sum() <= 2 and (not tie.any() or worst[tie].max() <= 5e-2)
            assert 10 * np.log10(1.0 / max(mse, 1e-20)) > 50
            assert abs(int(got["total"][0]) - ref["total_samples"]) <= max(4, 2e-3 * ref["total_samples"])
            worst_all.append(worst)
        if mode == "f16":
            outs_f16 = outs
        else:                                                                       # the fp16 hand-over is really on in the second pass
            assert not all(torch.equal(a, b) for a, b in zip(outs, outs_f16))


def test_config4_full_size_scoring_properties_and_oracle_views():
    """BASELINE config 4 at full size (256 candidate views x 4096 rays x 2 ensemble members, trained stand-ins): the pass is deterministic, a
    shard's rows equal the full pass's rows bit for bit (what lets the views shard over GPUs), every term is finite; eight of the views are
    rendered by the oracle for both members and scored by the oracle's scorer: the GPU's per-view terms follow within the tolerance the 1e-3
    render parity leaves (measured ~1e-4 relative)."""
    from apnrf_amd import render as RD
    from apnrf_amd import standin as SI
    from oracle import render as R
    from oracle import scorer as OS
    from oracle.field import FieldConfig, OracleField
    sc = H.make_scene("102344250", n_poses=40)
    members = [SI.train_standin(sc, DEV, steps=300, seed=s_) for s_ in (21, 22)]
    fields, ests = [m[0] for m in members], [m[1] for m in members]
    poses = SI._free_space_poses(sc, 256, seed=9)
    args = (640, 640, 320.0, 0.1, 1e-3, 0.1, 0.004, 0.01, DEV)
    terms, score = RD.score_views(fields, ests, poses, *args, group=False)
    terms2, _ = RD.score_views(fields, ests, poses, *args, group=False)
    assert terms.shape == (256, 4) and torch.isfinite(terms).all() and torch.equal(terms, terms2)
    part, _ = RD.score_views(fields, ests, poses[96:128], *args, group=False)
    assert torch.equal(part, terms[96:128])                                       # one rank's share of an 8-GPU run == those rows of the full pass
    assert abs(float(score) - float(RD.trajectory_score(terms))) < 1e-12
    cfg = FieldConfig(aabb=tuple(float(x) for x in sc["aabb"]), neurons=sc["neurons"], layers=sc["layers"], num_semantic_classes=sc["C"],
                      log2_hashmap_size=sc["log2_hashmap_size"])
    orcs = [OracleField(cfg, {"mlp_base": f.mlp_base.params.detach().cpu().numpy(), "mlp_head": f.mlp_head.params.detach().cpu().numpy(),
                              "mlp_sem": f.mlp_sem.params.detach().cpu().numpy()}, "f16", False) for f in fields]
    idx = R.subsample_indices(640 * 640, 4096)
    bk = torch.zeros(3)
    worst = 0.0
    for v in (0, 31, 64, 100, 129, 177, 222, 255):
        o, d = R.generate_image_rays(R.pose_to_c2w(poses[v]), 640, 640, 320.0, idx)
        rs = [R.render_prob_test(1024, orc, e.binaries.cpu().numpy(), sc["aabb"][None], o, d, render_bkgd=bk, **H.RENDER_KW) for orc, e in zip(orcs, ests)]
        st = lambda key, *s: np.stack([r[key].numpy().reshape(1, 1, 64, 64, *s) for r in rs])
        want = OS.per_view_terms(st("rgb_var", 3), st("depth_var"), st("acc"), st("sem", sc["C"]))[0]
        got = terms[v].cpu().numpy()
        rel = np.abs(got - want) / np.maximum(np.abs(want), 1e-2)
        print(f"config 4 view {v}: terms gpu {got} oracle {want} rel {rel}")
        worst = max(worst, float(rel.max()))
    assert worst < 2e-4, worst          # measured 2e-5 (profiles/r04_tests_full_size.txt)


# ------------------------------------------------------------------ tcnn's fp16 hash blend (mnf_field_config.blend_fp16)
@pytest.mark.parametrize("bf16", [False, True])
def test_field_fp16_blend_matches_its_oracle_and_differs_from_fp32_blend_as_expected(bf16):
    """`tcnn_blend_fp16=True`: the 8-corner blend as fp16 fused multiply-adds (tiny-cuda-nn's `fma((T)weight, value, result)`, T = __half)
    against the oracle restating exactly that (`blend="f16"`) at the default path's tolerances; and BOTH cross comparisons, so that the
    distance between the two blend precisions is on record: kernel fp16-blend vs oracle fp32-blend, kernel fp32-blend vs oracle fp16-blend."""
    sc = H.make_scene(log2_hashmap_size=15, head_gain=4.0)
    prec = "bf16" if bf16 else "f16"
    rng = np.random.default_rng(1)
    n = 5000 + 37
    a = sc["aabb"]
    pos = (rng.random((n, 3)) * (a[3:] - a[:3]) * 1.1 + a[:3] - 0.05 * (a[3:] - a[:3])).astype(np.float32)
    d = rng.normal(size=(n, 3)).astype(np.float32); d /= np.linalg.norm(d, axis=-1, keepdims=True)
    from oracle.field import FieldConfig, OracleField
    cfg = FieldConfig(aabb=tuple(float(x) for x in sc["aabb"]), neurons=sc["neurons"], layers=sc["layers"], num_semantic_classes=sc["C"],
                      log2_hashmap_size=sc["log2_hashmap_size"])
    outs, refs = {}, {}
    for blend in ("f32", "f16"):
        hip = H.hip_field(sc, mfma_bf16=bf16, tcnn_blend_fp16=(blend == "f16"))
        with torch.no_grad():
            outs[blend] = [t.cpu().numpy() for t in hip(torch.from_numpy(pos).to(DEV), torch.from_numpy(d).to(DEV))]
        refs[blend] = [t.numpy() for t in OracleField(cfg, sc["params"], prec, False, blend=blend)(torch.from_numpy(pos), torch.from_numpy(d))]
    inside = refs["f32"][1][:, 0] > 0
    tol = 8.0 if bf16 else 1.0

    def worst(got, want):
        return (float(np.abs(got[0][inside] - want[0][inside]).max()), float((np.abs(got[1] - want[1]) / (np.abs(want[1]) + 1e-6)).max()),
                float((np.abs(got[2][inside] - want[2][inside]) / (1.0 + np.abs(want[2][inside]))).max()))
    for kb in ("f32", "f16"):
        for ob in ("f32", "f16"):
            print(f"blend {prec}: kernel {kb} vs oracle {ob}: rgb max abs %.2e, sigma max rel %.2e, sem max err / (1 + |logit|) %.2e" % worst(outs[kb], refs[ob]))
    for b in ("f32", "f16"):           # each kernel mode against the oracle of ITS arithmetic: the default path's bars
        np.testing.assert_allclose(outs[b][1], refs[b][1], rtol=2e-3 * tol, atol=1e-6)
        np.testing.assert_allclose(outs[b][0][inside], refs[b][0][inside], atol=1e-3 * tol, rtol=0)
        np.testing.assert_allclose(outs[b][2][inside], refs[b][2][inside], atol=1e-3 * tol, rtol=2e-3 * tol)
    assert not np.array_equal(outs["f32"][2], outs["f16"][2])      # the switch does change the arithmetic
    # the two precisions are close to each other as well (features differ by fp16 rounding of the running sum): within 4x the bars
    x = worst(outs["f16"], refs["f32"])
    assert x[0] < 4e-3 * tol and x[1] < 1e-2 * tol and x[2] < 6e-3 * tol, x


def test_ensemble_members_on_their_own_streams_equal_sequential_steps():
    """`render.train_step_ensemble`: the members of an ensemble (pipeline.py:398-412 trains them one after the other) stepped side by side on one stream each give what
    stepping them in turn gives — same sample counts, same losses, parameters within float-atomics noise — and they do not share scratch (round 4: the cached workspace is
    per stream; with one per device two concurrent steps overwrote each other's samples)."""
    from apnrf_amd import render as RD
    from apnrf_amd.optim import FusedAdam
    sc = H.make_scene(log2_hashmap_size=15)
    bk = torch.tensor([0.3, 0.6, 0.1], device=DEV)
    data = []
    for m in range(2):
        o, d = H.view_rays(sc, 1 + m, h=40, w=40)
        rng = np.random.default_rng(50 + m)
        n = o.shape[0]
        data.append((RD.Rays(o.to(DEV), d.to(DEV)), torch.from_numpy(rng.random((n, 3)).astype(np.float32)).to(DEV),
                     torch.from_numpy(rng.uniform(0.5, 4.0, n).astype(np.float32)).to(DEV), torch.from_numpy(rng.integers(0, sc["C"], n)).to(DEV), bk))

    def run(concurrent):
        torch.manual_seed(5)
        mem = []
        for m in range(2):
            scm = H.make_scene(log2_hashmap_size=15, seed=m)
            f, e = H.hip_field(scm).train(), H.hip_estimator(scm)
            mem.append((f, e, FusedAdam(f.parameters(), lr=1e-3, eps=1e-15).bind_field(f)))
        hist = []
        for it in range(1, 7):
            if concurrent:
                outs = RD.train_step_ensemble(mem, data, step=it, stratified=False, **H.RENDER_KW)
            else:
                outs = [RD.train_step(f, e, o, *b, step=it, sync=False, stratified=False, **H.RENDER_KW) for (f, e, o), b in zip(mem, data)]
            hist.append(outs)
        torch.cuda.synchronize()
        return ([[int(o["n_rendering_samples"]) for o in outs] for outs in hist], [[float(o["loss"]) for o in outs] for outs in hist],
                [[int(o["skipped"]) for o in outs] for outs in hist], [[p.detach().clone() for p in f.parameters() if p.numel()] for f, _, _ in mem])
    n_a, l_a, s_a, p_a = run(False)
    n_b, l_b, s_b, p_b = run(True)
    assert n_a[0] == n_b[0] and min(n_a[0]) > 3000 and s_a == s_b and not any(any(x) for x in s_a)
    assert all(abs(x - y) <= max(3, 2e-3 * x) for ra, rb in zip(n_a, n_b) for x, y in zip(ra, rb))
    np.testing.assert_allclose(l_b, l_a, rtol=2e-3)
    for pa, pb in zip(p_a, p_b):
        for a, b in zip(pa, pb):
            assert torch.nn.functional.cosine_similarity(a, b, dim=0) > 0.9999
    assert len(RD._ENSEMBLE_STREAMS[torch.device(DEV)]) == 1                    # one extra stream, cached


def test_presampled_steps_are_bitwise_the_steps_that_march_themselves():
    """`render.presample` + `train_step(presampled=...)`: the march of batch k+1 runs on a side stream beside step k (`mnf_train_presample`), and the step that adopts it
    gives bit for bit what a step marching inside itself gives (deterministic accumulation, stratified near planes with the seed drawn at presample time) — through an
    occupancy refresh in the middle (the stale token is ignored, its seed is not), with a changing ray count, and asynchronously.  Also: the C side refuses a handle
    made for other rays."""
    import ctypes
    from apnrf_amd import _lib as L
    from apnrf_amd import render as RD
    from apnrf_amd.optim import FusedAdam
    sc = H.make_scene(log2_hashmap_size=15)
    bk = torch.tensor([0.3, 0.6, 0.1], device=DEV)
    steps = 9
    data = []
    for k in range(steps + 1):
        o, d = H.view_rays(sc, 1 + k % 3, h=36 + 2 * (k % 4), w=40)              # 1440 .. 1680 rays: the ray count changes from step to step
        rng = np.random.default_rng(70 + k)
        n = o.shape[0]
        data.append((RD.Rays(o.to(DEV), d.to(DEV)), torch.from_numpy(rng.random((n, 3)).astype(np.float32)).to(DEV),
                     torch.from_numpy(rng.uniform(0.5, 4.0, n).astype(np.float32)).to(DEV), torch.from_numpy(rng.integers(0, sc["C"], n)).to(DEV), bk))
    kw = dict(H.RENDER_KW)

    def run(pre, sync):
        f, e = H.hip_field(sc).train(), H.hip_estimator(sc)
        opt = FusedAdam(f.parameters(), lr=1e-3, eps=1e-15).bind_field(f)
        RD.reserve_sample_bounds(f, 1 << 21, 1 << 20)                             # no step overflows: same bounds (the deterministic grouping depends on them) in every run
        hist, tok, used = [], None, 0
        if pre:
            tok = RD.presample(f, e, data[0][0], seed=900 + 14, **kw)
        for k in range(steps):
            step = 14 + k                                                         # step 16 refreshes the occupancy grid: the tokens made before it (for steps 16 and 17) are stale
            nxt = RD.presample(f, e, data[k + 1][0], seed=900 + step + 1, **kw) if pre else None
            torch.manual_seed(1000 + step)                                        # (the refresh draws its cells from torch's generators)
            out = RD.train_step(f, e, opt, *data[k], step=step, sync=sync, deterministic=True, presampled=tok, seed=900 + step, **kw)
            used += int(tok is not None and tok.adopted)
            hist.append((out["loss"], out["n_rendering_samples"]))
            tok = nxt
        torch.cuda.synchronize()
        return [(float(l), int(n)) for l, n in hist], [p.detach().clone() for p in f.parameters() if p.numel()], used

    h_a, p_a, _ = run(False, True)
    for sync in (True, False):
        h_b, p_b, used = run(True, sync)
        assert used == steps - 2                                                  # adopted: every token but the two made in front of the refresh at step 16 (for steps 16 and 17)
        assert [n for _, n in h_a] == [n for _, n in h_b] and min(n for _, n in h_a) > 3000
        np.testing.assert_allclose([l for l, _ in h_b], [l for l, _ in h_a], rtol=1e-6)            # (the loss scalar is a float-atomic sum over ray blocks)
        for a, b in zip(p_a, p_b):
            assert torch.equal(a, b)
    # the loop helper: same trajectory again (jitter seeds differ from run to run here, so stratified=False), tokens adopted except around the refresh
    def run_helper(pre):
        f, e = H.hip_field(sc).train(), H.hip_estimator(sc)
        opt = FusedAdam(f.parameters(), lr=1e-3, eps=1e-15).bind_field(f)
        RD.reserve_sample_bounds(f, 1 << 21, 1 << 20)
        adopted, ns = 0, []
        src = RD.presampled_batches(data[:steps], f, e, first_step=14, stratified=False, **kw) if pre else ((14 + k, b, None) for k, b in enumerate(data[:steps]))
        for step, b, tok in src:
            torch.manual_seed(1000 + step)
            out = RD.train_step(f, e, opt, *b, step=step, sync=False, deterministic=True, stratified=False, presampled=tok, **kw)
            adopted += int(tok is not None and tok.adopted)
            ns.append(out["n_rendering_samples"])
        torch.cuda.synchronize()
        return [int(n) for n in ns], [p.detach().clone() for p in f.parameters() if p.numel()], adopted
    n_p, p_p, adopted = run_helper(True)
    n_q, p_q, _ = run_helper(False)
    assert adopted == steps - 3 and n_p == n_q and all(torch.equal(a, b) for a, b in zip(p_p, p_q))      # (no token for the first batch, none around step 16)
    # the C boundary: a handle made for other rays is refused (MNF_ERR_INVALID), not silently used
    f, e = H.hip_field(sc).train(), H.hip_estimator(sc)
    opt = FusedAdam(f.parameters(), lr=1e-3, eps=1e-15).bind_field(f)
    tok = RD.presample(f, e, data[1][0], **kw)
    tok.rays = (data[2][0].origins, data[2][0].viewdirs)
    tok.R = data[2][0].origins.shape[0]
    tok.cap_m = RD._train_state(f).caps(tok.R)[0]
    tok.keep = (L.contig(data[2][0].origins.reshape(-1, 3), torch.float32),) + tuple(tok.keep[1:])
    with pytest.raises(L.MnfError, match="presampled was made for other rays"):
        RD.train_step(f, e, opt, *data[2], step=3, deterministic=True, presampled=tok, **kw)


def test_async_scheduler_counts_optimizer_updates_not_calls():
    """`train_step(sync=False)` advances the LR scheduler at every call, also for iterations the device-side guard skipped; the reference `continue`s before
    `optimizer.step()` / `scheduler.step()` (pipeline.py:491, :520-532).  The step's final skip flag now travels to the host with its counts, and a skipped step gives its
    scheduler step back one or two calls later: after the run the scheduler has stepped once per optimizer update."""
    from apnrf_amd import render as RD
    from apnrf_amd.optim import FusedAdam
    sc = H.make_scene(log2_hashmap_size=15)
    bk = torch.tensor([0.3, 0.6, 0.1], device=DEV)
    o, d = H.view_rays(sc, 1, h=40, w=40)
    rng = np.random.default_rng(3)
    n = o.shape[0]
    batch = (RD.Rays(o.to(DEV), d.to(DEV)), torch.from_numpy(rng.random((n, 3)).astype(np.float32)).to(DEV),
             torch.from_numpy(rng.uniform(0.5, 4.0, n).astype(np.float32)).to(DEV), torch.from_numpy(rng.integers(0, sc["C"], n)).to(DEV), bk)
    f, e = H.hip_field(sc).train(), H.hip_estimator(sc)
    opt = FusedAdam(f.parameters(), lr=1e-3, eps=1e-15).bind_field(f)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=1, gamma=0.99)
    st = RD._train_state(f)
    st.by_R[n] = (1 << 18, 64)                                                  # a surviving-sample bound every early step overflows: skipped on the device, the bound grows late
    outs = [RD.train_step(f, e, opt, *batch, step=1 + k, sync=False, stratified=False, scheduler=sched, **H.RENDER_KW) for k in range(12)]
    torch.cuda.synchronize()
    skipped = sum(int(o_["skipped"]) > 0 for o_ in outs)
    updates = int(opt.state[f.mlp_base.params]["step"].item()) if "step" in opt.state[f.mlp_base.params] else None
    assert 1 <= skipped <= 4 and updates == 12 - skipped
    # flags of the last one or two steps may still be in flight at the last call: settle them with calls that cannot skip
    for k in range(3):
        outs.append(RD.train_step(f, e, opt, *batch, step=20 + k, sync=False, stratified=False, scheduler=sched, **H.RENDER_KW))
    torch.cuda.synchronize()
    assert not any(int(o_["skipped"]) for o_ in outs[12:])
    assert st.skipped_steps == skipped and st.sched_debt == 0
    assert sched.last_epoch == 15 - skipped                                        # one scheduler step per optimizer update
    np.testing.assert_allclose(opt.param_groups[0]["lr"], 1e-3 * 0.99 ** (15 - skipped), rtol=1e-6)


def test_presampled_step_beyond_its_marched_bound_is_skipped_like_a_step_that_marches_itself():
    """The bound check of the march runs inside the presample (its own counters) and the adopting step copies them: a batch that marches more samples than `max_marched`
    must come out of a presampled step exactly as out of a plain one — skip flag raised, status bit 1, the marched count reported, zero gradients, parameters untouched —
    and the bounds must grow from the late report as they do without a presample."""
    from apnrf_amd import render as RD
    from apnrf_amd.optim import FusedAdam
    sc = H.make_scene(log2_hashmap_size=15)
    bk = torch.tensor([0.3, 0.6, 0.1], device=DEV)
    o, d = H.view_rays(sc, 2, h=40, w=40)
    rng = np.random.default_rng(5)
    n = o.shape[0]
    batch = (RD.Rays(o.to(DEV), d.to(DEV)), torch.from_numpy(rng.random((n, 3)).astype(np.float32)).to(DEV),
             torch.from_numpy(rng.uniform(0.5, 4.0, n).astype(np.float32)).to(DEV), torch.from_numpy(rng.integers(0, sc["C"], n)).to(DEV), bk)
    res = []
    for pre in (False, True):
        f, e = H.hip_field(sc).train(), H.hip_estimator(sc)
        opt = FusedAdam(f.parameters(), lr=1e-3, eps=1e-15).bind_field(f)
        st = RD._train_state(f)
        st.by_R[n] = (4096, 1 << 20)                                            # far fewer marched samples than this batch has
        p0 = [p.detach().clone() for p in f.parameters() if p.numel()]
        tok = RD.presample(f, e, batch[0], seed=7, stratified=False, **H.RENDER_KW) if pre else None
        out = RD.fused_forward_backward(f, e, *batch[:4], render_bkgd=bk, sync=False, stratified=False, presampled=tok, seed=7, **H.RENDER_KW)
        torch.cuda.synchronize()
        assert (tok.adopted if pre else True)
        counts, skip = out["counts"].tolist(), int(out["skip"])
        g = [float(p.grad.abs().max()) for p in f.parameters() if p.numel()]
        res.append((counts, skip, g))
        assert skip >= 1 and counts[3] & 1 and counts[0] > 4096 and counts[1] == 0 and max(g) == 0.0
        opt.step(skip=out["skip"], count_nonfinite=True)
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(p0, [p.detach() for p in f.parameters() if p.numel()]))
        # the late report grows the bounds: the next step of the same batch fits
        tok = RD.presample(f, e, batch[0], seed=8, stratified=False, **H.RENDER_KW) if pre else None
        out2 = RD.fused_forward_backward(f, e, *batch[:4], render_bkgd=bk, sync=False, stratified=False, presampled=tok, seed=8, **H.RENDER_KW)
        torch.cuda.synchronize()
        assert int(out2["skip"]) == 0 and int(out2["counts"][1]) > 3000 and int(out2["counts"][0]) == counts[0]
    assert res[0][0] == res[1][0] and res[0][1] == res[1][1]


def test_feature_rows_are_bitwise_a_second_gather():
    """The training forward reads every survivor's encoded features from the row the density pre-pass left (`FieldIO::rows_in`) instead of gathering 128 table
    entries again: same bits as the two-gather form, which only the diag build can still run (MNF_NO_ROWS): child process (tests/diag_rows.py), fp16 and bf16."""
    import os
    import subprocess
    import sys
    from apnrf_amd import build as B
    here = os.path.dirname(os.path.abspath(__file__))
    assert os.path.exists(B.LIB_DIAG), "libmi355nerf_diag.so missing: run `python __graft_entry__.py build`"
    env = dict(os.environ, MNF_LIB_PATH=B.LIB_DIAG)
    r = subprocess.run([sys.executable, os.path.join(here, "diag_rows.py")], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "DIAG_ROWS_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def test_composite_backward_without_per_sample_rgb_sem_gradients():
    """`mnf_composite_train_backward` with d_rgbs = d_sems = NULL (the caller forms weight x per-ray gradient itself, as the train step's backward-data kernel does):
    d_sigmas is bit for bit what the full call writes, and the products the caller would form equal the arrays of the full call."""
    import ctypes
    from apnrf_amd import _lib as L
    lib = L.load_library()
    rng = np.random.default_rng(8)
    R, C = 300, 29
    cnts = rng.integers(0, 200, R)
    cnts[::17] = 0
    starts = np.concatenate([[0], np.cumsum(cnts)[:-1]])
    N = int(cnts.sum())
    cu = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    ts = np.sort(rng.random(N).astype(np.float32)) * 3
    te = ts + rng.uniform(1e-3, 2e-2, N).astype(np.float32)
    sig, rgb, sem = rng.uniform(0, 30, N).astype(np.float32), rng.random((N, 3)).astype(np.float32), rng.normal(size=(N, C)).astype(np.float32)
    d = dict(starts=cu(starts.astype(np.int64)), cnts=cu(cnts.astype(np.int64)), ts=cu(ts), te=cu(te), sig=cu(sig), rgb=cu(rgb), sem=cu(sem), bk=cu(np.array([0.2, 0.4, 0.6], np.float32)))
    o_rgb, o_acc, o_dep, o_sem = torch.empty(R, 3, device=DEV), torch.empty(R, device=DEV), torch.empty(R, device=DEV), torch.empty(R, C, device=DEV)
    w, tr = torch.empty(N, device=DEV), torch.empty(N, device=DEV)
    L.launch(lib.mnf_composite_train_forward, L.ptr(d["starts"]), L.ptr(d["cnts"]), R, L.ptr(d["ts"]), L.ptr(d["te"]), L.ptr(d["sig"]), L.ptr(d["rgb"]), L.ptr(d["sem"]), C, N,
             L.ptr(d["bk"]), L.ptr(o_rgb), L.ptr(o_acc), L.ptr(o_dep), L.ptr(o_sem), L.ptr(w), L.ptr(tr), None)
    g_rgb, g_dep, g_sem = cu(rng.normal(size=(R, 3)).astype(np.float32)), cu(rng.normal(size=R).astype(np.float32)), cu(rng.normal(size=(R, C)).astype(np.float32))
    outs = []
    for full in (True, False):
        ds, dr, dm = torch.zeros(N, device=DEV), torch.zeros(N, 3, device=DEV), torch.zeros(N, C, device=DEV)
        L.launch(lib.mnf_composite_train_backward, L.ptr(d["starts"]), L.ptr(d["cnts"]), R, L.ptr(d["ts"]), L.ptr(d["te"]), L.ptr(d["sig"]), L.ptr(d["rgb"]), L.ptr(d["sem"]), C, N,
                 L.ptr(d["bk"]), L.ptr(w), L.ptr(tr), L.ptr(o_acc), L.ptr(o_dep), L.ptr(g_rgb), None, L.ptr(g_dep), L.ptr(g_sem), L.ptr(ds),
                 L.ptr(dr) if full else None, L.ptr(dm) if full else None)
        outs.append((ds, dr, dm))
    torch.cuda.synchronize()
    assert torch.equal(outs[0][0], outs[1][0]) and float(outs[0][0].abs().max()) > 0
    ray = torch.repeat_interleave(torch.arange(R, device=DEV), d["cnts"])
    assert torch.equal(outs[0][1], w[:, None] * g_rgb[ray]) and torch.equal(outs[0][2], w[:, None] * g_sem[ray])


def test_optimizer_step_report_writes_counters_and_final_skip_flag_to_pinned_memory():
    """`mnf_field_optimizer_step_report` (through `FusedAdam.step(report=...)`): the train step's four device counters and the FINAL skip flag — the non-finite count of
    this very call included — land in pinned host memory without a copy on the stream; the update itself is the plain call's."""
    from apnrf_amd.optim import FusedAdam
    sc = H.make_scene(log2_hashmap_size=15)
    res = []
    for report in (False, True):
        torch.manual_seed(3)
        f = H.hip_field(sc).train()
        opt = FusedAdam(f.parameters(), lr=1e-2, eps=1e-15).bind_field(f)
        for p in f.parameters():
            if p.numel():
                p.grad = torch.randn_like(p) * 1e-3
        counts = torch.tensor([123456, 7890, 321, 0], dtype=torch.int64, device=DEV)
        skip = torch.zeros((), dtype=torch.int32, device=DEV)
        host = torch.full((5,), -1, dtype=torch.int64).pin_memory()
        opt.step(skip=skip, count_nonfinite=True, report=(counts, host) if report else None)
        torch.cuda.synchronize()
        assert opt.reported == report
        if report:
            assert host.tolist() == [123456, 7890, 321, 0, 0]
        res.append([p.detach().clone() for p in f.parameters() if p.numel()])
        # a non-finite gradient: the flag is raised by this call's own count, reported, and nothing moves
        f.mlp_head.params.grad[5] = float("nan")
        before = [p.detach().clone() for p in f.parameters() if p.numel()]
        skip.zero_()
        opt.step(skip=skip, count_nonfinite=True, report=(counts, host) if report else None)
        torch.cuda.synchronize()
        assert int(skip) >= 1 and all(torch.equal(a, b) for a, b in zip(before, [p.detach() for p in f.parameters() if p.numel()]))
        if report:
            assert host.tolist()[:4] == [123456, 7890, 321, 0] and host[4].item() == int(skip)
    assert all(torch.equal(a, b) for a, b in zip(*res))
