"""The yardstick of the predictive-information map tests: a numpy float64 restatement of the four per-pixel terms of
`ActiveNeRFMapper.probablistic_uncertainty` (scripts/pipeline.py:727-774) BEFORE the np.mean that collapses each of them
(:735 / :746 / :760 / :773), on member-major stacks rgb_var [M,V,P,3], depth_var [M,V,P], acc [M,V,P], sem [M,V,P,C]; the per-view
means of those maps; and the scaling to 8 bits that `mnf_score_view_maps` documents for its heat bytes.  Pure numpy: no GPU, no
package import.

Checked against tests/golden/scorer.npz (test_infomap_cpu.py): the mean of the maps over all views and pixels, weighted 1 / 1 / 3 / 2,
is the reference's own `terms`, and the per-view means are `oracle.scorer.per_view_terms`, both far inside 1e-12."""
import numpy as np

WEIGHTS = np.array([1.0, 1.0, 3.0, 2.0])       # pipeline.py:775-781
K2PIE = 2 * np.pi * np.e


def _softmax(x):
    x = x - x.max(axis=-1, keepdims=True)
    e = np.exp(x)
    return e / e.sum(axis=-1, keepdims=True)


def _gauss_information(var):
    """pipeline.py:727-735 / :737-746 without the outer mean: `var` [M, ...] -> [...].  The ensemble variance is sum / 2 whatever M is."""
    ce = np.log(K2PIE * var + 1e-4) / 2
    ens = np.sum(var, axis=0) / 2
    return np.log(K2PIE * ens + 1e-4) / 2 - np.mean(ce, axis=0)


def maps(rgb_var, depth_var, acc, sem):
    """[V,P,4] float64: rgb (mean over the three channels), depth, semantic, occupancy of every pixel.  NaN / inf propagate."""
    rgb_var, depth_var, acc, sem = (np.asarray(a, np.float64) for a in (rgb_var, depth_var, acc, sem))
    with np.errstate(all="ignore"):
        rgb = np.mean(_gauss_information(rgb_var), axis=-1)
        dep = _gauss_information(depth_var)
        p = _softmax(sem)
        s_ce = -np.sum((p + 1e-4) * np.log(p + 1e-4), axis=-1)
        p_ens = np.mean(p, axis=0)
        s = -np.sum((p_ens + 1e-4) * np.log(p_ens + 1e-4), axis=-1) - np.mean(s_ce, axis=0)
        o_ce = -(acc + 1e-4) * np.log(acc + 1e-4) - (1 - acc + 1e-4) * np.log(1 - acc + 1e-4)
        a_ens = np.mean(acc, axis=0)
        o = -(a_ens + 1e-4) * np.log(a_ens + 1e-4) - (1 - a_ens + 1e-4) * np.log(1 - a_ens + 1e-4) - np.mean(o_ce, axis=0)
    return np.stack([rgb, dep, s, o], axis=-1)


def terms_of_maps(m):
    """[V,P,4] -> [V,4]: the per-view means (un-weighted)."""
    with np.errstate(all="ignore"):
        return np.asarray(m, np.float64).mean(axis=1)


def terms(rgb_var, depth_var, acc, sem):
    return terms_of_maps(maps(rgb_var, depth_var, acc, sem))


def sat8(x):
    """Narrow to uint8 as frames_ref.sat8: clamp to [0, 255], round to nearest with ties to even, NaN -> 0."""
    x = np.asarray(x, np.float64)
    with np.errstate(invalid="ignore"):
        r = np.rint(np.clip(x, 0, 255))
    return np.where(np.isnan(r), 0, r).astype(np.uint8)


def heat(m, lo, hi):
    """sat8(((x - lo_k) / (hi_k - lo_k)) * 255.0) on float64 maps [...,4], every operation rounded on its own, in that order."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    with np.errstate(all="ignore"):
        return sat8(((np.asarray(m, np.float64) - lo) / (hi - lo)) * 255.0)
