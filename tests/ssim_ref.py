"""The yardstick of the structural-similarity tests: a numpy float64 restatement of the definition `mnf_ssim_views` documents
(include/mi355nerf.h) — Wang et al.'s SSIM with the 11-tap, sigma 1.5 Gaussian window over the VALID windows only, what
`skimage.metrics.structural_similarity(gaussian_weights=True, sigma=1.5, use_sample_covariance=False, data_range=L, channel_axis=-1)`
returns after its border crop and what mip-NeRF's `compute_ssim` computes.  Pure numpy: no GPU, no package import.

Checked against a `scipy.ndimage.gaussian_filter` form of skimage's algorithm (test_ssim_cpu.py) to 1e-12."""
import numpy as np

WINDOW, SIGMA, K1, K2 = 11, 1.5, 0.01, 0.03
HALO = WINDOW - 1


def weights():
    """g[i] = exp(-0.5 ((i - 5) / 1.5)^2), i = 0 .. 10, normalised to sum 1."""
    g = np.exp(-0.5 * ((np.arange(WINDOW, dtype=np.float64) - WINDOW // 2) / SIGMA) ** 2)
    return g / g.sum()


def _valid_filter(a, g):
    """[..., H, W, K] -> [..., H - 10, W - 10, K]: rows (along W) first, then columns, taps added in index order, no padding."""
    H, W = a.shape[-3], a.shape[-2]
    rows = g[0] * a[..., :, 0:W - HALO, :]
    for k in range(1, WINDOW):
        rows = rows + g[k] * a[..., :, k:k + W - HALO, :]
    out = g[0] * rows[..., 0:H - HALO, :, :]
    for k in range(1, WINDOW):
        out = out + g[k] * rows[..., k:k + H - HALO, :, :]
    return out


def channel_maps(x, y, data_range=1.0, k1=K1, k2=K2):
    """S_c at every window centre: x, y [..., H, W, K] (any float dtype, widened to float64) -> [..., H - 10, W - 10, K].
    NaN / inf propagate."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    assert x.shape == y.shape and x.shape[-3] >= WINDOW and x.shape[-2] >= WINDOW
    g = weights()
    c1, c2 = (k1 * data_range) ** 2, (k2 * data_range) ** 2
    with np.errstate(all="ignore"):
        mx, my = _valid_filter(x, g), _valid_filter(y, g)
        exx, eyy, exy = _valid_filter(x * x, g), _valid_filter(y * y, g), _valid_filter(x * y, g)
        vx, vy, cxy = exx - mx * mx, eyy - my * my, exy - mx * my
        return ((2 * mx * my + c1) * (2 * cxy + c2)) / ((mx * mx + my * my + c1) * (vx + vy + c2))


def ssim(x, y, data_range=1.0, k1=K1, k2=K2):
    """x, y [V, H, W, K] -> (score [V], map [V, H - 10, W - 10]): the map is (S_0 + ... + S_{K-1}) / K, the score the sum of S_c over
    centres and channels divided by their number."""
    s = channel_maps(x, y, data_range, k1, k2)
    with np.errstate(all="ignore"):
        m = s[..., 0]
        for c in range(1, s.shape[-1]):
            m = m + s[..., c]
        return s.reshape(s.shape[0], -1).sum(axis=1) / (s.shape[1] * s.shape[2] * s.shape[3]), m / s.shape[-1]
