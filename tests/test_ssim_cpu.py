"""CPU-side checks of the structural-similarity pass (`mnf_ssim_views`, csrc/ssim.hip; render.ssim_views / ssim_metrics): the numpy
restatement the GPU tests are held to (tests/ssim_ref.py) against a `scipy.ndimage.gaussian_filter` form of skimage's
`structural_similarity(gaussian_weights=True, sigma=1.5, use_sample_covariance=False)` with its border crop of 5, at 1e-12; known
answers; and the entry points' symbols and refusals, which need the built library but no device."""
import ctypes
import os
import re

import numpy as np
import pytest

import apnrf_amd
import ssim_ref as SR
from apnrf_amd import _lib as L

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")


def _images(h, w, k, seed):
    """Smooth structure plus noise, as float32 values: a pair that is neither identical nor unrelated."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = 0.5 + 0.3 * np.sin(xx / 3.1)[..., None] * np.cos(yy / 4.7)[..., None] + 0.1 * rng.standard_normal((h, w, k))
    x = np.clip(base, 0, 1).astype(np.float32)
    y = np.clip(base + 0.08 * rng.standard_normal((h, w, k)), 0, 1).astype(np.float32)
    return x, y


def _scipy_form(x, y, data_range):
    """skimage's algorithm: gaussian_filter (sigma 1.5, truncate 3.5 -> radius 5, mode 'reflect') per channel, then crop 5."""
    ndi = pytest.importorskip("scipy.ndimage")
    x, y = x.astype(np.float64), y.astype(np.float64)
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    out = np.empty((x.shape[0] - 10, x.shape[1] - 10, x.shape[2]))
    for c in range(x.shape[2]):
        f = lambda a: ndi.gaussian_filter(a, sigma=1.5, truncate=3.5, mode="reflect")
        ux, uy = f(x[..., c]), f(y[..., c])
        vx, vy, vxy = f(x[..., c] ** 2) - ux * ux, f(y[..., c] ** 2) - uy * uy, f(x[..., c] * y[..., c]) - ux * uy
        s = ((2 * ux * uy + c1) * (2 * vxy + c2)) / ((ux ** 2 + uy ** 2 + c1) * (vx + vy + c2))
        out[..., c] = s[5:-5, 5:-5]
    return out


@pytest.mark.parametrize("h, w, k", [(11, 11, 3), (12, 27, 1), (67, 131, 3)])
def test_restatement_equals_the_scipy_form(h, w, k):
    x, y = _images(h, w, k, h * w)
    for data_range in (1.0, 2.5):
        want = _scipy_form(x, y, data_range)
        got = SR.channel_maps(x, y, data_range)
        assert got.shape == (h - 10, w - 10, k)
        print(f"{h}x{w}x{k} L={data_range}: max |restatement - scipy form| = {np.abs(got - want).max():.3e}, map range [{want.min():.4f}, {want.max():.4f}]")
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)
        score, m = SR.ssim(x[None], y[None], data_range)
        np.testing.assert_allclose(score[0], want.mean(), rtol=0, atol=1e-12)
        np.testing.assert_allclose(m[0], want.mean(-1), rtol=0, atol=1e-12)
        assert 0.0 < want.min() and want.max() < 0.999               # the pair is neither identical nor unrelated


def test_weights():
    g = SR.weights()
    assert g.shape == (11,) and abs(g.sum() - 1.0) < 1e-15 and np.array_equal(g, g[::-1]) and g.argmax() == 5
    np.testing.assert_allclose(g[5] / g[4], np.exp(0.5 / 2.25), rtol=1e-14)


def test_identical_inputs_give_exactly_one():
    rng = np.random.default_rng(5)
    for x in (rng.random((2, 23, 31, 3)).astype(np.float32), (0.9 + 0.01 * rng.random((1, 11, 40, 1))).astype(np.float32),
              (rng.random((1, 14, 12, 4)) * 37.0).astype(np.float32)):
        score, m = SR.ssim(x, x, data_range=1.0)
        assert (SR.channel_maps(x, x) == 1.0).all() and (m == 1.0).all() and (score == 1.0).all()


def test_constant_images_known_answer():
    for a, b, L_ in ((0.25, 0.75, 1.0), (0.0, 1.0, 1.0), (3.0, 4.0, 10.0)):
        x, y = np.full((1, 13, 17, 2), a, np.float32), np.full((1, 13, 17, 2), b, np.float32)
        c1 = (0.01 * L_) ** 2
        want = (2 * a * b + c1) / (a * a + b * b + c1)
        score, m = SR.ssim(x, y, data_range=L_)
        np.testing.assert_allclose(m, want, rtol=0, atol=1e-12)
        np.testing.assert_allclose(score, want, rtol=0, atol=1e-12)


def test_a_nan_pixel_covers_its_windows_only():
    x, y = (a[None] for a in _images(30, 33, 3, 1))
    x = x.copy()
    x[0, 12, 20, 1] = NAN
    x[0, 2, 3, 0] = NAN                                           # near the corner: clipped footprint
    score, m = SR.ssim(x, y)
    want = np.zeros((20, 23), bool)
    want[2:13, 10:21] = True                                      # centres r with r <= 12 <= r + 10
    want[0:3, 0:4] = True
    assert np.array_equal(np.isnan(m[0]), want) and np.isnan(score[0])


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
    for name in ("mnf_ssim_views", "mnf_ssim_views_workspace_bytes"):
        assert re.search(r"\b%s\s*\(" % name, code), f"{name} is not declared in include/mi355nerf.h"
        assert hasattr(raw, name), f"{name} is not exported"
        assert name in L.SIGNATURES and hasattr(lib, name)
    res, args = L.SIGNATURES["mnf_ssim_views"]
    assert res is ctypes.c_int32 and len(args) == 17                          # 16 arguments + the stream
    assert args[4] is ctypes.c_int64 and args[15] is ctypes.c_int64           # pixels_per_image and workspace_bytes are 64-bit
    assert args[9:12] == [ctypes.c_double] * 3                                # data_range, k1, k2
    assert L.SIGNATURES["mnf_ssim_views_workspace_bytes"] == (ctypes.c_int64, [ctypes.c_int32] * 4)
    assert re.search(r"#define\s+MNF_SSIM_WINDOW\s+11\b", code) and re.search(r"#define\s+MNF_SSIM_MAX_CHANNELS\s+4\b", code)
    assert "pipeline.py:550-613" in header
    from apnrf_amd import render as RD
    assert (RD.SSIM_WINDOW, RD.SSIM_SIGMA, RD.SSIM_K1, RD.SSIM_K2) == (11, 1.5, 0.01, 0.03) == (SR.WINDOW, SR.SIGMA, SR.K1, SR.K2)


def test_workspace_bytes(lib):
    ws = lib.mnf_ssim_views_workspace_bytes
    assert ws(3, 11, 11, 3) == 3 * 8                              # one window: one tile: one partial sum per view
    assert ws(1, 18, 42, 1) == 8 and ws(1, 19, 42, 1) == 16 and ws(1, 18, 43, 4) == 16       # tiles of 8 x 32 centres
    assert ws(2, 67, 131, 3) == 2 * 8 * 4 * 8                     # 57 x 121 centres: 8 x 4 tiles
    assert ws(2, 800, 800, 3) == 2 * 512 * 8                      # 99 x 25 tiles: the run count is capped
    assert ws(1, 800, 800, 1) == ws(1, 800, 800, 4)               # the plan does not depend on K
    assert ws(0, 11, 11, 3) == 0
    assert ws(-1, 11, 11, 3) == 0 and ws(1, 10, 11, 3) == 0 and ws(1, 11, 10, 3) == 0 and ws(1, 11, 11, 0) == 0 and ws(1, 11, 11, 5) == 0


def _call(lib, **over):
    """mnf_ssim_views with plausible (never dereferenced) device pointers; `over` replaces arguments by name."""
    a = dict(pred=0x1000, target_f32=0x2000, target_u8=None, image_ids=None, pixels_per_image=0, n_views=2, height=20, width=30, channels=3,
             data_range=1.0, k1=0.01, k2=0.03, ssim=0x5000, map=0x6000, workspace=0x8000, workspace_bytes=1 << 20, stream=None)
    assert not set(over) - set(a)
    a.update(over)
    rc = lib.mnf_ssim_views(*a.values())
    return rc, lib.mnf_last_error().decode()


U8 = dict(target_f32=None, target_u8=0x3000, image_ids=0x4000, pixels_per_image=600)

BAD_ARGUMENTS = [
    (dict(height=10), "11"), (dict(width=10), "11"), (dict(height=0), "11"), (dict(width=-3), "11"),
    (dict(channels=0), "channels"), (dict(channels=5), "channels"), (dict(channels=-1), "channels"),
    (dict(target_u8=0x3000, image_ids=0x4000, pixels_per_image=600), "exactly one"), (dict(target_f32=None), "exactly one"),
    (dict(U8, channels=1), "channels == 3"), (dict(U8, pixels_per_image=599), "pixels_per_image"), (dict(U8, image_ids=None), "image_ids"),
    (dict(data_range=0.0), "data_range"), (dict(data_range=-1.0), "data_range"), (dict(data_range=NAN), "data_range"), (dict(data_range=INF), "data_range"),
    (dict(k1=-0.01), "k1"), (dict(k1=NAN), "k1"), (dict(k2=-1e-9), "k2"), (dict(k2=INF), "k2"),
    (dict(ssim=None), "ssim is null"), (dict(ssim=0x5004), "ssim"), (dict(map=0x6004), "map"), (dict(map=0x6001), "map"),
    (dict(pred=None), "pred"), (dict(pred=0x1002), "4-byte"), (dict(target_f32=0x2001), "4-byte"),
    (dict(workspace_bytes=15), "workspace too small"), (dict(workspace_bytes=0), "workspace too small"), (dict(workspace=None), "workspace"),
    (dict(workspace=0x8004), "workspace"),
    (dict(height=800, width=800, workspace_bytes=2 * 512 * 8 - 1), "workspace too small"),
    (dict(n_views=65536, workspace_bytes=1 << 30), "65535"), (dict(n_views=-1), "n_views"),
]


@pytest.mark.parametrize("over, word", BAD_ARGUMENTS)
def test_refuses_bad_argument(lib, over, word):
    rc, msg = _call(lib, **over)
    assert rc == -1 and word in msg, (rc, msg)


def test_accepts_zero_views(lib):
    rc, msg = _call(lib, n_views=0)
    assert rc == 0, msg
    rc, msg = _call(lib, n_views=0, pred=None, ssim=None, map=None, workspace=None, workspace_bytes=0)
    assert rc == 0, msg
    rc, msg = _call(lib, n_views=0, height=10)                    # the sizes are checked first
    assert rc == -1, msg


def test_python_surface_refuses_before_touching_a_device():
    import torch
    from apnrf_amd import render as RD
    r = lambda *s: torch.zeros(*s)
    with pytest.raises(ValueError, match="one shape"):
        RD.ssim_views(r(2, 12, 12, 3), r(2, 12, 13, 3))
    with pytest.raises(ValueError, match="one shape"):
        RD.ssim_views(r(12, 12), r(12, 12))
    with pytest.raises(ValueError, match="channels"):
        RD.ssim_views(r(1, 12, 12, 5), r(1, 12, 12, 5))
    with pytest.raises(ValueError, match="at least that size"):
        RD.ssim_views(r(1, 10, 12, 3), r(1, 10, 12, 3))
    for bad in (0.0, -1.0, NAN, INF):
        with pytest.raises(ValueError, match="data_range"):
            RD.ssim_views(r(1, 12, 12, 3), r(1, 12, 12, 3), data_range=bad)
    with pytest.raises(L.MnfError, match="GPU tensors only"):
        RD.ssim_views(r(1, 12, 12, 3), r(1, 12, 12, 3))
