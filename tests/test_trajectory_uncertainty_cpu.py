"""The ensemble-disagreement trajectory scorer (`ActiveNeRFMapper.trajector_uncertainty`, scripts/pipeline.py:800-916) without a GPU:
a float64 numpy restatement of its reduction (pipeline.py:861-896), written from the formulas and pinned to the RUNNING reference by
tests/golden/trajectory.npz (generator: tests/golden/make_golden_trajectory.py), and the host-side helpers of `apnrf_amd.render`.
The GPU tests (test_gpu_trajectory_uncertainty.py) compare the kernel with this restatement."""
import numpy as np


def ensemble_rows(rgb, depth, acc, sem):
    """The four clipped rows [4,V] float64 of pipeline.py:861-882.  rgb [M,V,P,3], depth [M,V,P], acc [M,V,P] (member 0 is read),
    sem [S,V,P,C]; any float dtype, widened to float64 first."""
    rgb, depth, acc, sem = (np.asarray(a, np.float64) for a in (rgb, depth, acc, sem))
    z = sem - sem.max(-1, keepdims=True)
    p = np.exp(z) / np.exp(z).sum(-1, keepdims=True)                  # the float64 softmax
    entropy = -(p * np.log(p + 1e-10)).sum(-1)                        # [S,V,P]
    rgb_var = ((rgb - rgb.mean(0)) ** 2).mean(0).mean(-1)             # population variance over the members, then the channel mean: [V,P]
    depth_var = ((depth - depth.mean(0)) ** 2).mean(0)
    with np.errstate(divide="ignore"):
        acc_inv = np.clip(1.0 / (acc[0] + 1e-4) - 1.0, 0.0, 10000.0)  # per pixel, before the mean
    return np.stack([np.clip(rgb_var.mean(-1) * 4000.0, 0.0, 100.0), np.clip(depth_var.mean(-1) * 50.0, 0.0, 100.0), acc_inv.mean(-1),
                     np.clip(entropy.mean((0, 2)) * 50.0, 0.0, 100.0)])


def uncertainty_of_rows(rows, step):
    """pipeline.py:883-896 on the [4,V] rows."""
    per_view = rows[0] + rows[1] + rows[2] + rows[3]
    return float(np.mean(per_view[-11:]) if step == -1 else np.mean(per_view))


def golden_stacks(g):
    """member-major [M,V,P,.] float64 stacks of the reference's own renders (V = 40 views of 5 x 5 pixels, two members; member 0's logits)"""
    st = lambda nm: np.stack([g[f"m{m}_{nm}"].astype(np.float64) for m in range(2)])
    rgb, depth, acc = st("images"), st("depths"), st("accs")
    V = rgb.shape[1]
    return rgb.reshape(2, V, -1, 3), depth.reshape(2, V, -1), acc.reshape(2, V, -1), g["m0_sems"].astype(np.float64).reshape(1, V, rgb.shape[2] * rgb.shape[3], -1)


def test_restatement_equals_running_reference(golden):
    g = golden("trajectory")
    rgb, depth, acc, sem = golden_stacks(g)
    assert rgb.shape == (2, 40, 25, 3) and sem.shape == (1, 40, 25, 29) and g["rows"].shape == (4, 40)
    rows = ensemble_rows(rgb, depth, acc, sem)
    np.testing.assert_allclose(rows, g["rows"], rtol=1e-12)
    np.testing.assert_allclose(uncertainty_of_rows(rows, 1), float(g["unc_step1"]), rtol=1e-12)
    np.testing.assert_allclose(uncertainty_of_rows(rows, -1), float(g["unc_stepm1"]), rtol=1e-12)
    # what the golden covers: unclipped rgb / depth rows, an acc row with exact zeros, a semantic row that is clipped everywhere
    assert (g["rows"][0] < 100).all() and (g["rows"][1] < 100).all() and (g["rows"][2] == 0).any() and (g["rows"][3] == 100.0).all()


def test_trajectory_view_indices_equal_reference(golden):
    from apnrf_amd import render as RD
    g = golden("trajectory")
    idx = RD.trajectory_view_indices(len(g["trajectory"]))
    assert len(g["trajectory"]) == 60 and idx.shape == (40,)
    np.testing.assert_array_equal(idx, g["unc_idx"])


def test_uncertainty_from_terms_equals_reference(golden):
    import torch
    from apnrf_amd import render as RD
    g = golden("trajectory")
    terms = np.ascontiguousarray(g["rows"].T)
    for t in (terms, torch.from_numpy(terms)):
        for step, key in ((1, "unc_step1"), (-1, "unc_stepm1")):
            unc, max_idx = RD.trajectory_uncertainty_from_terms(t, step)
            np.testing.assert_allclose(unc, float(g[key]), rtol=1e-12)
            np.testing.assert_array_equal(max_idx, np.arange(40))
            np.testing.assert_array_equal(max_idx, g["max_idx"])
    assert float(g["unc_step1"]) != float(g["unc_stepm1"])
