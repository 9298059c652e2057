"""The oracle's render loops, train render and sampler away from the yaml's render options, against what the RUNNING reference answered
(tests/golden/glue_options.npz, written by tests/golden/make_golden.py gen_glue_options; scene, field, rays and background are glue_ngp.npz's):

  R1..R6  utils.py:555-779 / :782-1032 at the options of tests/test_gpu_render_options.py: cone angle 0 (round budgets 1, 2, 3), no alpha threshold,
          early_stop_eps 0 and 0.2, near / far planes inside the box, a threshold that drops two thirds of the samples, a budget that ends the render
  T1..T6  occ_grid.py:80-238 at the options of tests/test_gpu_train_options.py; utils.py:63-219 (eval mode) at T1, T4 and T5: the reference function
          has no `early_stop_eps` argument, so T2, T6 (eps 0) and T3 (eps 0.2) exist for the sampler only

CPU only.  Bars as tests/test_glue_golden_cpu.py: round schedules, counts and sample sets bit-exact, floating point 1e-6."""
import numpy as np
import pytest
import torch

import helpers as H  # noqa: F401  (registers the package alias)
from test_glue_golden_cpu import _close, _t, ngp_oracle_fields, scene_of


def _kw(g, tag):
    pre = tag + "_kw_"
    return {k[len(pre):]: float(g[k]) for k in g.files if k.startswith(pre)}


@pytest.fixture(scope="module")
def setup(golden):
    base, g = golden("glue_ngp"), golden("glue_options")
    (f, _), = ngp_oracle_fields(base, [int(base["param_seed"])])
    return g, scene_of(base), f, _t(base["rays_o"]), _t(base["rays_d"]), _t(base["bkgd"])


def test_fixture_options_are_the_gpu_tests_options(golden):
    """The fixture pins the oracle at the very options the GPU tests compare the kernels with it at."""
    import test_gpu_render_options as TR
    import test_gpu_train_options as TT
    g = golden("glue_options")
    for tag in ("R1", "R2", "R3", "R4", "R5", "R6"):
        kw, max_samples = TR.CASES[tag][:2]
        assert _kw(g, tag) == {k: float(v) for k, v in kw.items()} and int(g[tag + "_max_samples"]) == max_samples, tag
    for tag, kw in TT.CASES.items():
        assert _kw(g, tag) == {k: float(v) for k, v in kw.items()}, tag


@pytest.mark.parametrize("tag", ["R1", "R2", "R3", "R4", "R5", "R6"])
def test_oracle_test_renderers_equal_reference_at_options(setup, tag):
    from oracle import render as R
    g, sc, f, o, d, bk = setup
    out = R.render_prob_test(int(g[tag + "_max_samples"]), f, sc["occ"], sc["aabb"][None], o, d, render_bkgd=bk, **_kw(g, tag))
    det = R.render_test(int(g[tag + "_max_samples"]), f, sc["occ"], sc["aabb"][None], o, d, render_bkgd=bk, **_kw(g, tag))
    assert [list(r) for r in out["rounds"]] == g[tag + "_rounds"].tolist() == [list(r) for r in det["rounds"]]      # (rays alive, samples per ray) of every round
    assert out["total_samples"] == det["total_samples"] == int(g[tag + "_total"])
    for k in ("rgb", "acc", "depth", "rgb_var", "depth_var"):
        _close(out[k].numpy(), g[f"{tag}_{k}"], f"{tag}_{k}")
    _close(out["sem"].numpy()[:, ::2], g[tag + "_sem_every2"], tag + "_sem")
    for k in ("rgb", "acc", "depth", "sem"):
        assert torch.equal(det[k], out[k]), k                      # the reference's two loops agreed bit for bit (asserted by the generator): so do the oracle's
    strides = {int(s) for _, s in out["rounds"]}
    if tag == "R1":
        assert {1, 2, 3} <= strides
    if tag == "R2":
        assert out["alive_at_end"] > 0 and sum(s for _, s in out["rounds"]) >= 200      # the budget ended the render, not the rays
    if tag == "R6":
        assert sum(s for _, s in out["rounds"]) == 52              # utils.py:666-672: the loop tests the budget before a round, not inside it


@pytest.mark.parametrize("tag", ["T1", "T2", "T3", "T4", "T5", "T6"])
def test_oracle_sampling_and_train_render_equal_reference_at_options(setup, tag):
    from oracle import render as R
    g, sc, f, o, d, bk = setup
    kw = _kw(g, tag)
    near = torch.full((len(o),), kw.pop("near_plane"))

    def sigma_fn(ts, te, ri):
        return f.query_density(o[ri] + d[ri] * (ts + te)[:, None] / 2.0).squeeze(-1)
    ri, ts, te, n_all = R.sampling(sc["occ"], sc["aabb"][None], sc["occs_mean"], o, d, sigma_fn, near, **kw)
    assert n_all == int(g[tag + "_samp_all_n"])
    np.testing.assert_array_equal(np.bincount(ri.numpy(), minlength=len(o)), g[tag + "_samp_cnt"])
    assert float(ts.double().sum()) == float(g[tag + "_samp_ts_sum"]) and float(te.double().sum()) == float(g[tag + "_samp_te_sum"])
    if tag == "T2":
        assert len(ri) == n_all                                     # no filter at all
    if tag == "T5":
        assert sc["occs_mean"] < kw["alpha_thre"]                   # occ_grid.py:199: the mean decides
    if tag + "_tre_n" not in g.files:
        assert tag in ("T2", "T3", "T6")                                  # no `early_stop_eps` on utils.py:63-80
        return
    with torch.no_grad():
        rgb, acc, depth, sem, n, _ = R.render_train(f, sc["occ"], sc["aabb"][None], sc["occs_mean"], o, d, near, render_bkgd=bk, **kw)
    assert n == int(g[tag + "_tre_n"]) == len(ri)
    for got, k in ((rgb, "rgb"), (acc, "acc"), (depth, "depth")):
        _close(got.numpy(), g[f"{tag}_tre_{k}"], k)
    _close(sem.numpy()[:, ::4], g[tag + "_tre_sem_every4"], "sem")
