"""CPU-side checks of the per-pixel predictive-information maps (`mnf_score_view_maps`, csrc/infomap.hip; render.view_information_maps /
score_view_maps): the numpy restatement the GPU tests are held to (tests/infomap_ref.py) against the RUNNING reference's recorded
scorer (tests/golden/scorer.npz) and against the oracle's per-view terms, both at 1e-12 (the bar oracle/scorer.py is held to); known
answers of the 8-bit scaling; and the entry points' symbols and refusals, which need the built library but no device."""
import ctypes
import os
import re

import numpy as np
import pytest

import apnrf_amd
import infomap_ref as IR
from apnrf_amd import _lib as L

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")


def golden_stacks(g):
    """member-major [M,V,P,.] float64 stacks of the reference's own probabilistic renders (two members, 40 views of 5 x 5 pixels)"""
    st = lambda nm: np.stack([g[f"m{m}_{nm}"].astype(np.float64) for m in range(2)])
    rv, dv, ac, sm = st("images_var"), st("depths_var"), st("accs"), st("sems")
    V = rv.shape[1]
    return rv.reshape(2, V, -1, 3), dv.reshape(2, V, -1), ac.reshape(2, V, -1), sm.reshape(2, V, dv.shape[2] * dv.shape[3], -1)


def test_restatement_equals_running_reference(golden):
    g = golden("scorer")
    rv, dv, ac, sm = golden_stacks(g)
    assert rv.shape == (2, 40, 25, 3) and sm.shape == (2, 40, 25, 29)
    assert (ac > 1.0).any()                                   # an opacity of 1 + 2.4e-7 is legal: 1 - a + 1e-4 stays positive
    m = IR.maps(rv, dv, ac, sm)
    assert m.shape == (40, 25, 4) and np.isfinite(m).all()
    weighted = m.reshape(-1, 4).mean(0) * IR.WEIGHTS
    print("restatement vs golden terms:", np.abs(weighted - g["terms"]).max(), " vs pi:", abs(weighted.sum() - float(g["pi"])))
    np.testing.assert_allclose(weighted, g["terms"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(weighted.sum(), float(g["pi"]), rtol=0, atol=1e-12)
    np.testing.assert_allclose((IR.terms(rv, dv, ac, sm) * IR.WEIGHTS).sum(1).mean(), float(g["pi"]), rtol=0, atol=1e-12)


def test_restatement_equals_oracle_per_view_terms(golden):
    from oracle import scorer as SC
    g = golden("scorer")
    rv, dv, ac, sm = golden_stacks(g)
    o6 = lambda a: a.reshape(2, 1, 40, 5, 5, *a.shape[3:])    # the oracle's [M,1,V,h,w,.] layout (pipeline.py:720-725)
    ref = SC.per_view_terms(o6(rv), o6(dv), o6(ac), o6(sm))
    got = IR.terms(rv, dv, ac, sm)
    print("restatement vs oracle per-view terms:", np.abs(got - ref).max())
    np.testing.assert_allclose(got, ref, rtol=0, atol=1e-12)
    # M = 3: the / 2 of pipeline.py:733 stays a / 2
    rng = np.random.default_rng(2)
    rv3, dv3 = rng.random((3, 2, 7, 3)) ** 4, rng.random((3, 2, 7)) ** 4
    ac3, sm3 = rng.random((3, 2, 7)), rng.normal(size=(3, 2, 7, 5)) * 3
    o6 = lambda a: a.reshape(3, 1, 2, 7, 1, *a.shape[3:])
    np.testing.assert_allclose(IR.terms(rv3, dv3, ac3, sm3), SC.per_view_terms(o6(rv3), o6(dv3), o6(ac3), o6(sm3)), rtol=0, atol=1e-12)


def test_identical_members_carry_no_information_but_the_rgb_quirk():
    rng = np.random.default_rng(3)
    one = (rng.random((1, 2, 9, 3)), rng.random((1, 2, 9)), rng.random((1, 2, 9)), rng.normal(size=(1, 2, 9, 6)))
    m = IR.maps(*(np.repeat(a, 2, axis=0) for a in one))
    assert np.abs(m).max() < 1e-14                            # sum / 2 of two equal variances is that variance
    m3 = IR.maps(*(np.repeat(a, 3, axis=0) for a in one))
    assert np.abs(m3[..., 2:]).max() < 1e-14 and m3[..., :2].min() > 0.1      # sum / 2 of three is 1.5 x: log(1.5) / 2 = 0.2027


def test_nan_and_inf_stay_in_their_pixel():
    rng = np.random.default_rng(4)
    rv, dv, ac, sm = rng.random((2, 1, 6, 3)), rng.random((2, 1, 6)), rng.random((2, 1, 6)), rng.normal(size=(2, 1, 6, 4))
    clean = IR.maps(rv, dv, ac, sm)
    rv[0, 0, 1, 2] = NAN; dv[1, 0, 2] = NAN; ac[0, 0, 3] = NAN; sm[1, 0, 4, 0] = INF; sm[0, 0, 5, 1] = -INF
    m = IR.maps(rv, dv, ac, sm)
    want = np.zeros((6, 4), bool)
    want[1, 0] = want[2, 1] = want[3, 3] = want[4, 2] = True  # +inf - max = NaN; -inf is a class of probability 0
    assert (np.isnan(m[0]) == want).all()
    assert np.array_equal(m[0][~want & (np.arange(6) != 5)[:, None]], clean[0][~want & (np.arange(6) != 5)[:, None]])
    assert np.isnan(IR.terms_of_maps(m)).tolist() == [[True, True, True, True]]


def test_heat_known_answers():
    assert IR.sat8([0.5, 1.5, 2.5, 254.5, 255.5, 300.0, INF, -3.0, -INF, NAN, 0.0, 255.0]).tolist() == [0, 2, 2, 254, 255, 255, 255, 0, 0, 0, 0, 255]
    assert IR.sat8([1.0]).dtype == np.uint8
    x = np.array([[0.0, 1.0, -1.0, 0.5], [2.0, 3.0, 1.0, 0.25], [NAN, INF, -INF, 0.1], [1.0, 2.0, 0.0, 0.7]])
    h = IR.heat(x, [0.0, 1.0, -1.0, 0.0], [2.0, 3.0, 1.0, 1.0])
    # 0.5 * 255 = 127.5 -> 128 (even); 0.25 * 255 = 63.75; 0.1 * 255 = 25.5 -> 26 (even); 0.7 * 255 = 178.49999999999997
    assert h.tolist() == [[0, 0, 0, 128], [255, 255, 255, 64], [0, 255, 0, 26], [128, 128, 128, 178]]
    # a reversed range reverses the ramp; values outside the range saturate
    assert IR.heat(np.array([[0.0, 0.5, 2.0, -1.0]]), [1.0] * 4, [0.0] * 4).tolist() == [[255, 128, 0, 255]]


# ------------------------------------------------------------------ the entry points, without a device
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as G
    G.build()
    return apnrf_amd.load_library()


def test_symbols_declared_exported_and_bound(lib):
    header = open(os.path.join(REPO, "include", "mi355nerf.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    raw = ctypes.CDLL(L.lib_path())
    for name in ("mnf_score_view_maps", "mnf_score_view_maps_workspace_bytes"):
        assert re.search(r"\b%s\s*\(" % name, code), f"{name} is not declared in include/mi355nerf.h"
        assert hasattr(raw, name), f"{name} is not exported"
        assert name in L.SIGNATURES and hasattr(lib, name)
    res, args = L.SIGNATURES["mnf_score_view_maps"]
    assert res is ctypes.c_int32 and len(args) == 16                          # 15 arguments + the stream
    assert args[6] is ctypes.c_int64 and args[14] is ctypes.c_int64           # n_pix and workspace_bytes are 64-bit
    assert L.SIGNATURES["mnf_score_view_maps_workspace_bytes"] == (ctypes.c_int64, [ctypes.c_int32, ctypes.c_int64, ctypes.c_int32])
    assert re.search(r"#define\s+MNF_SCORE_MAPS_MAX_MEMBERS\s+64\b", code) and re.search(r"#define\s+MNF_SCORE_MAPS_MAX_CLASSES\s+1024\b", code)
    assert "pipeline.py:727-774" in header
    from apnrf_amd import render as RD
    assert (RD.SCORE_MAPS_MAX_MEMBERS, RD.SCORE_MAPS_MAX_CLASSES) == (64, 1024)


def test_workspace_bytes(lib):
    ws = lib.mnf_score_view_maps_workspace_bytes
    assert ws(3, 25, 29) == 3 * 1 * 32                        # one tile per view: one row of four partial sums
    assert ws(2, 185, 29) == 2 * 2 * 32                       # 184 pixels per tile at 29 classes
    assert ws(1, 40, 1024) == 10 * 32                         # 4 pixels per tile at the class maximum
    assert ws(2, 131372, 3) == 2 * 512 * 32                   # 514 tiles of 256: the run count is capped
    assert ws(0, 25, 29) == 0
    assert ws(-1, 25, 29) == 0 and ws(1, 0, 29) == 0 and ws(1, 25, 0) == 0 and ws(1, 25, 1025) == 0


LO, HI = (ctypes.c_double * 4)(0.0, 0.0, 0.0, 0.0), (ctypes.c_double * 4)(1.0, 1.0, 1.0, 1.0)


def _call(lib, **over):
    """mnf_score_view_maps with plausible (never dereferenced) device pointers; `over` replaces arguments by name."""
    a = dict(rgb_var=0x1000, depth_var=0x2000, acc=0x3000, sem=0x4000, n_members=2, n_views=2, n_pix=64, n_classes=29, terms=0x5000, maps=0x6000,
             heat8=0x7000, lo=LO, hi=HI, workspace=0x8000, workspace_bytes=1 << 20, stream=None)
    assert not set(over) - set(a)
    a.update(over)
    rc = lib.mnf_score_view_maps(*a.values())
    return rc, lib.mnf_last_error().decode()


def _d4(*x):
    return (ctypes.c_double * 4)(*x)


@pytest.mark.parametrize("over, word", [
    (dict(n_members=0), "n_members"), (dict(n_members=-1), "n_members"), (dict(n_views=-1), "n_views"), (dict(n_pix=0), "n_pix"),
    (dict(n_pix=-7), "n_pix"), (dict(n_classes=0), "n_classes"), (dict(n_classes=-2), "n_classes"),
    (dict(terms=None, maps=None, heat8=None), "nothing to compute"),
    (dict(lo=None), "ranges"), (dict(hi=None), "ranges"), (dict(lo=None, hi=None), "ranges"),
    (dict(hi=_d4(1.0, 1.0, 0.0, 1.0)), "empty"), (dict(lo=_d4(0.0, 2.5, 0.0, 0.0), hi=_d4(1.0, 2.5, 1.0, 1.0)), "empty"),
    (dict(lo=_d4(0.0, 0.0, 0.0, -0.0), hi=_d4(1.0, 1.0, 1.0, 0.0)), "empty"),
    (dict(lo=_d4(NAN, 0.0, 0.0, 0.0)), "finite"), (dict(hi=_d4(1.0, INF, 1.0, 1.0)), "finite"), (dict(lo=_d4(0.0, 0.0, -INF, 0.0)), "finite"),
    (dict(maps=0x6004), "maps"), (dict(maps=0x6001), "maps"), (dict(heat8=0x7002), "heat8"), (dict(heat8=0x7001), "heat8"),
    (dict(terms=0x5004), "terms"),
    (dict(rgb_var=None), "null"), (dict(depth_var=None), "null"), (dict(acc=None), "null"), (dict(sem=None), "null"),
    (dict(sem=0x4002), "4-byte"), (dict(acc=0x3001), "4-byte"),
    (dict(workspace_bytes=63), "workspace too small"), (dict(workspace_bytes=0), "workspace too small"), (dict(workspace=None), "workspace"),
    (dict(workspace=0x8004), "workspace"),
    (dict(n_pix=131372, n_classes=3, workspace_bytes=2 * 512 * 32 - 1), "workspace too small"),
    (dict(n_views=65536, workspace_bytes=1 << 30), "65535"),
])
def test_refuses_bad_argument(lib, over, word):
    rc, msg = _call(lib, **over)
    assert rc == -1 and word in msg, (rc, msg)


@pytest.mark.parametrize("over", [dict(n_members=65), dict(n_classes=1025), dict(n_members=1000, n_classes=4096)])
def test_unsupported_above_the_maxima(lib, over):
    rc, msg = _call(lib, **over)
    assert rc == -3 and "supported 64 members of 1024 classes" in msg, (rc, msg)


def test_accepts_zero_views(lib):
    rc, msg = _call(lib, n_views=0)
    assert rc == 0, msg
    rc, msg = _call(lib, n_views=0, rgb_var=None, depth_var=None, acc=None, sem=None, terms=None, maps=None, heat8=None, lo=None, hi=None, workspace=None,
                    workspace_bytes=0)
    assert rc == 0, msg
    rc, msg = _call(lib, n_views=0, n_classes=1025)           # the limits are checked first
    assert rc == -3, msg


def test_python_surface_refuses_before_touching_a_device():
    import torch
    from apnrf_amd import render as RD
    r = lambda *s: torch.zeros(*s)
    M, V, P, C = 2, 3, 8, 4
    with pytest.raises(ValueError, match=r"\[M,V,P,3\]"):
        RD.view_information_maps(r(M, V, P, 4), r(M, V, P), r(M, V, P), r(M, V, P, C))
    with pytest.raises(ValueError, match=r"\[M,V,P,3\]"):
        RD.view_information_maps(r(M, V, P, 3), r(M, V, P), r(M, V, P), r(V, P, C))
    with pytest.raises(ValueError, match="do not match"):
        RD.view_information_maps(r(M, V, P, 3), r(M, V, P + 1), r(M, V, P), r(M, V, P, C))
    with pytest.raises(ValueError, match="do not match"):
        RD.view_information_maps(r(M, V, P, 3), r(M, V, P), r(1, V, P), r(M, V, P, C))
    with pytest.raises(ValueError, match="do not match"):
        RD.view_information_maps(r(M + 1, V, P, 3), r(M, V, P), r(M, V, P), r(M, V, P, C))
    with pytest.raises(ValueError, match="supported 64 members"):
        RD.view_information_maps(r(65, 1, 2, 3), r(65, 1, 2), r(65, 1, 2), r(65, 1, 2, C))
    with pytest.raises(ValueError, match="supported 64 members"):
        RD.view_information_maps(r(1, 1, 2, 3), r(1, 1, 2), r(1, 1, 2), r(1, 1, 2, 1025))
    with pytest.raises(ValueError, match="at least one"):
        RD.view_information_maps(r(M, V, 0, 3), r(M, V, 0), r(M, V, 0), r(M, V, 0, C))
    good = (r(M, V, P, 3), r(M, V, P), r(M, V, P), r(M, V, P, C))
    with pytest.raises(ValueError, match="heat_range"):
        RD.view_information_maps(*good, heat_range=([0.0] * 3, [1.0] * 3))
    with pytest.raises(ValueError, match="heat_range"):
        RD.view_information_maps(*good, heat_range=([0.0, 0.0, 1.0, 0.0], [1.0, 1.0, 1.0, 1.0]))
    with pytest.raises(ValueError, match="heat_range"):
        RD.view_information_maps(*good, heat_range=([0.0] * 4, [1.0, NAN, 1.0, 1.0]))
    with pytest.raises(L.MnfError, match="GPU tensors only"):
        RD.view_information_maps(*good)
