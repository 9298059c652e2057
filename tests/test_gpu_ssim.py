"""GPU tests of the structural-similarity pass: `mnf_ssim_views` (csrc/ssim.hip) through `render.ssim_views` / `render.ssim_metrics`,
and `render.evaluate_views(ssim=True)`.

The yardstick is tests/ssim_ref.py, the numpy float64 restatement of the definition in include/mi355nerf.h (held to the scipy form of
skimage's algorithm at 1e-12 by test_ssim_cpu.py), on the same fp32 values; bar rtol 1e-9 / atol 1e-12, the bar tests/test_gpu_eval.py
holds `mnf_eval_views` to: both sides are double-precision evaluations of the same expressions on the same inputs, in the same order."""
import functools

import numpy as np
import pytest
import torch

import helpers as H
import ssim_ref as SR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RTOL, ATOL = 1e-9, 1e-12
C = 29
N_IMAGES = 3
SENTINEL = -12345.678


@functools.lru_cache(maxsize=None)
def _case(h, w, k, v=3):
    """(x, y) [v,h,w,k] fp32 CPU tensors — smooth structure plus noise, so that the maps spread over (0, 1) — and the restatement's
    (score [v], map [v,h-10,w-10]).  Computed once per shape; nobody writes to them."""
    rng = np.random.default_rng(1000 * h + 10 * w + k)
    yy, xx = np.mgrid[0:h, 0:w]
    base = 0.5 + 0.3 * (np.sin(xx / 3.1) * np.cos(yy / 4.7))[None, ..., None] + 0.1 * rng.standard_normal((v, h, w, k))
    x = np.clip(base, 0, 1).astype(np.float32)
    y = np.clip(base + 0.08 * rng.standard_normal((v, h, w, k)), 0, 1).astype(np.float32)
    return torch.from_numpy(x), torch.from_numpy(y), SR.ssim(x, y)


def _bits(t):
    return t.view(torch.int64)


def _check(got, want_score, want_map, what):
    score, m = got["ssim"].cpu().numpy(), got["maps"].cpu().numpy()
    print(f"{what}: ssim {score} want {want_score} max abs diff {np.nanmax(np.abs(score - want_score)):.3e}; map max abs diff "
          f"{np.nanmax(np.abs(m - want_map)):.3e}, map range [{np.nanmin(want_map):.4f}, {np.nanmax(want_map):.4f}]")
    np.testing.assert_allclose(score, want_score, rtol=RTOL, atol=ATOL, equal_nan=True, err_msg=what)
    np.testing.assert_allclose(m, want_map, rtol=RTOL, atol=ATOL, equal_nan=True, err_msg=what)


@pytest.mark.parametrize("h, w, k", [(11, 11, 1), (11, 11, 3),                      # one window
                                     (12, 27, 1), (12, 27, 3), (12, 27, 4),          # 2 x 17 centres: non-square, odd, one short tile
                                     (67, 131, 1), (67, 131, 3),                     # 57 x 121 centres: ragged against the 8 x 32 tile both ways, 8 x 4 tiles
                                     (200, 160, 1), (200, 160, 3)])                  # 120 workgroups per view
def test_matches_restatement(h, w, k):
    from apnrf_amd import render as RD
    x, y, (want_score, want_map) = _case(h, w, k)
    got = RD.ssim_views(x.to(DEV), y.to(DEV), maps=True)
    assert got["ssim"].is_cuda and got["ssim"].dtype == torch.float64 and tuple(got["ssim"].shape) == (3,)
    assert got["maps"].dtype == torch.float64 and tuple(got["maps"].shape) == (3, h - 10, w - 10)
    assert np.isfinite(want_map).all() and want_map.max() < 0.999
    _check(got, want_score, want_map, f"{h}x{w}x{k}")
    only = RD.ssim_views(x.to(DEV), y.to(DEV))
    assert only["maps"] is None and torch.equal(_bits(only["ssim"]), _bits(got["ssim"]))
    if k == 1:                                                   # a [V,H,W] plane is K = 1
        plane = RD.ssim_views(x[..., 0].to(DEV), y[..., 0].to(DEV), maps=True)
        assert torch.equal(_bits(plane["ssim"]), _bits(got["ssim"])) and torch.equal(_bits(plane["maps"]), _bits(got["maps"]))


def test_data_range_scales_the_constants():
    """Depth against depth: values in metres with data_range = the span."""
    from apnrf_amd import render as RD
    x, y, _ = _case(12, 27, 1)
    x6, y6 = x * 6.0, y * 6.0
    got = RD.ssim_views(x6.to(DEV), y6.to(DEV), data_range=6.0, maps=True)
    _check(got, *SR.ssim(x6.numpy(), y6.numpy(), data_range=6.0), what="12x27x1 data_range 6")


@pytest.fixture(scope="module")
def scene():
    return H.make_scene(log2_hashmap_size=15)


@pytest.fixture(scope="module")
def dataset(scene, tmp_path_factory):
    """`Dataset(training=False)` of 48 x 40 random u8 images (as test_gpu_eval.py builds them), every label inside [0, C)."""
    from apnrf_amd import render as RD
    from apnrf_amd.dataset import Dataset
    rng = np.random.default_rng(1)
    h, w = 48, 40
    c2w = np.stack([RD.pose_to_c2w(np.asarray(p, np.float64)) for p in scene["poses"][:N_IMAGES]]).astype(np.float32)
    ds = Dataset(training=False, save_fp=str(tmp_path_factory.mktemp("ssim") / "plain"), device=DEV)
    ds.update_data(rng.integers(0, 256, size=(N_IMAGES, h, w, 3), dtype=np.uint8), rng.uniform(0.2, 6.0, size=(N_IMAGES, h, w)).astype(np.float32),
                   rng.integers(0, C, size=(N_IMAGES, h, w)).astype(np.int64), c2w)
    return ds


def test_dataset_route(dataset):
    from apnrf_amd import render as RD
    h, w = dataset.height, dataset.width
    ids = [2, 0, 1]
    pixels = torch.stack([dataset[i]["pixels"] for i in ids])                        # [3,h,w,3] fp32: (float)u8 / 255.0f
    assert tuple(pixels.shape) == (3, h, w, 3)
    g = torch.Generator().manual_seed(3)
    rgb = (pixels.cpu() + 0.3 * torch.randn(3, h, w, 3, generator=g)).clamp(0, 1)
    want = SR.ssim(rgb.numpy(), pixels.cpu().numpy())
    got = RD.ssim_metrics(rgb.to(DEV), dataset, ids, maps=True)
    _check(got, *want, what="dataset 48x40")
    assert 0.05 < want[0].min() and want[0].max() < 0.95
    flat = RD.ssim_metrics(rgb.view(3, h * w, 3).to(DEV), dataset, torch.tensor(ids), maps=True)      # the [V,P,3] form, ids as a host tensor
    assert torch.equal(_bits(flat["ssim"]), _bits(got["ssim"])) and torch.equal(_bits(flat["maps"]), _bits(got["maps"]))
    same = RD.ssim_views(rgb.to(DEV), pixels, maps=True)                            # u8 storage and its fp32 pixels are the same target
    assert torch.equal(_bits(same["ssim"]), _bits(got["ssim"])) and torch.equal(_bits(same["maps"]), _bits(got["maps"]))
    exact = RD.ssim_metrics(pixels, dataset, ids, maps=True)
    assert (exact["ssim"] == 1.0).all() and (exact["maps"] == 1.0).all()
    with pytest.raises(IndexError):
        RD.ssim_metrics(rgb.to(DEV), dataset, [0, 1, N_IMAGES])
    with pytest.raises(ValueError):
        RD.ssim_metrics(rgb[:, :, :-1].to(DEV), dataset, ids)


@pytest.mark.parametrize("h, w, k", [(12, 27, 4), (67, 131, 3), (200, 160, 1)])
def test_identical_images_give_exactly_one(h, w, k):
    from apnrf_amd import render as RD
    x = _case(h, w, k)[0].to(DEV)
    got = RD.ssim_views(x, x, maps=True)
    assert (got["ssim"] == 1.0).all() and (got["maps"] == 1.0).all()


def _into(RD, x, y, ssim, maps, **kw):
    V, h, w, k = x.shape
    RD._ssim_into(x, y, None, None, 0, V, h, w, k, 1.0, ssim, maps, **kw)


@pytest.mark.parametrize("h, w, k", [(12, 27, 3), (67, 131, 3), (67, 131, 1)])
def test_unaligned_planes_and_guard_bands(h, w, k):
    """Planes that start 1 and 3 floats past a 16-byte boundary (the staging takes a scalar head up to the first boundary of the address)
    give the bits of the same values in tensors of their own, and nothing outside `ssim` and `map` is written: both sit inside larger
    buffers of sentinels, `map` 8 bytes off the 16-byte grid."""
    from apnrf_amd import render as RD
    x, y, _ = _case(h, w, k)
    own = [x.to(DEV), y.to(DEV)]
    shifted = []
    for off, t in zip((1, 3), own):
        flat = torch.full((t.numel() + 8,), float("nan"), device=DEV)                # a read outside the plane would poison the result
        view = flat[off:off + t.numel()].view(t.shape)
        view.copy_(t)
        assert view.is_contiguous() and t.data_ptr() % 16 == 0 and view.data_ptr() % 16 == 4 * off
        shifted.append(view)
    want = RD.ssim_views(*own, maps=True)
    n_map, pad = 3 * (h - 10) * (w - 10), 67
    score_buf = torch.full((3 + 2 * pad,), SENTINEL, dtype=torch.float64, device=DEV)
    map_buf = torch.full((n_map + 2 * pad,), SENTINEL, dtype=torch.float64, device=DEV)
    score, m = score_buf[pad:pad + 3], map_buf[pad:pad + n_map].view(3, h - 10, w - 10)
    assert m.data_ptr() % 16 == 8
    _into(RD, *shifted, score, m)
    assert torch.equal(_bits(score), _bits(want["ssim"])) and torch.equal(_bits(m), _bits(want["maps"]))
    for buf, n in ((score_buf, 3), (map_buf, n_map)):
        assert (buf[:pad] == SENTINEL).all() and (buf[pad + n:] == SENTINEL).all()


def test_a_views_bits_do_not_depend_on_the_call():
    from apnrf_amd import render as RD
    x, y, _ = _case(67, 131, 3)
    x, y = x.to(DEV), y.to(DEV)
    a = RD.ssim_views(x, y, maps=True)
    b = RD.ssim_views(x, y, maps=True)
    assert torch.equal(_bits(a["ssim"]), _bits(b["ssim"])) and torch.equal(_bits(a["maps"]), _bits(b["maps"]))
    alone = RD.ssim_views(x[1:2], y[1:2], maps=True)
    first = RD.ssim_views(x[[1, 0, 2]], y[[1, 0, 2]], maps=True)
    last = RD.ssim_views(x[[2, 0, 1]], y[[2, 0, 1]], maps=True)
    for r, pos in ((alone, 0), (first, 0), (last, 2)):
        assert torch.equal(_bits(r["ssim"])[pos], _bits(a["ssim"])[1]) and torch.equal(_bits(r["maps"])[pos], _bits(a["maps"])[1])


def test_nan_covers_its_windows_and_stays_in_its_view():
    from apnrf_amd import render as RD
    x, y, _ = _case(67, 131, 3)
    clean = RD.ssim_views(x.to(DEV), y.to(DEV), maps=True)
    xn = x.clone()
    xn[1, 30, 70, 2] = float("nan")                               # interior: the full 11 x 11 footprint, across tile borders both ways
    want_score, want_map = SR.ssim(xn.numpy(), y.numpy())
    assert np.isnan(want_map[1]).sum() == 121 and np.isnan(want_map[1, 20:31, 60:71]).all()
    got = RD.ssim_views(xn.to(DEV), y.to(DEV), maps=True)
    m = got["maps"].cpu().numpy()
    assert np.array_equal(np.isnan(m), np.isnan(want_map))
    score = got["ssim"].cpu().numpy()
    assert np.isnan(score[1]) and np.isfinite(score[[0, 2]]).all()
    _check(got, want_score, want_map, what="67x131x3 with a NaN")
    for v in (0, 2):
        assert torch.equal(_bits(got["ssim"])[v], _bits(clean["ssim"])[v]) and torch.equal(_bits(got["maps"])[v], _bits(clean["maps"])[v])
    keep = ~np.isnan(want_map[1])
    assert np.array_equal(m[1][keep], clean["maps"].cpu().numpy()[1][keep])


def test_argument_errors_raise_and_enqueue_nothing(dataset):
    from apnrf_amd import _lib as L
    from apnrf_amd import render as RD
    lib = L.load_library()
    x, y, _ = _case(12, 27, 3)
    x, y = x.to(DEV), y.to(DEV)
    V, h, w, k = x.shape
    score = torch.full((V,), SENTINEL, dtype=torch.float64, device=DEV)
    maps = torch.full((V, h - 10, w - 10), SENTINEL, dtype=torch.float64, device=DEV)
    ws = torch.zeros(1 << 12, dtype=torch.uint8, device=DEV)
    ids = torch.arange(V, dtype=torch.int64, device=DEV)
    odd = L.DevPtr(maps.data_ptr() + 4)
    odd.device = maps.device
    nan, inf = float("nan"), float("inf")

    def call(**over):
        a = dict(pred=L.ptr(x), target_f32=L.ptr(y), target_u8=None, image_ids=None, pixels_per_image=0, n_views=V, height=h, width=w, channels=k,
                 data_range=1.0, k1=0.01, k2=0.03, ssim=L.ptr(score), map=L.ptr(maps), workspace=L.ptr(ws), workspace_bytes=ws.numel())
        assert not set(over) - set(a)
        a.update(over)
        L.launch(lib.mnf_ssim_views, *a.values())

    u8 = dict(target_f32=None, target_u8=L.ptr(dataset.images), image_ids=L.ptr(ids), pixels_per_image=h * w)
    for over in (dict(height=10, width=32), dict(height=30, width=10), dict(channels=0), dict(channels=5),
                 dict(target_u8=L.ptr(dataset.images), image_ids=L.ptr(ids), pixels_per_image=h * w), dict(target_f32=None),
                 dict(u8, channels=1), dict(u8, pixels_per_image=h * w + 1),
                 dict(data_range=0.0), dict(data_range=-1.0), dict(data_range=nan), dict(data_range=inf),
                 dict(k1=-0.01), dict(k1=nan), dict(k1=inf), dict(k2=-0.03), dict(k2=nan), dict(k2=inf),
                 dict(ssim=None), dict(map=odd), dict(workspace_bytes=V * 8 - 1), dict(n_views=65536)):
        with pytest.raises(L.MnfError):
            call(**over)
    torch.cuda.synchronize()
    assert (score == SENTINEL).all() and (maps == SENTINEL).all()
    call(n_views=0)                                               # fine, and writes nothing
    torch.cuda.synchronize()
    assert (score == SENTINEL).all() and (maps == SENTINEL).all()
    empty = RD.ssim_views(x[:0], y[:0], maps=True)
    assert tuple(empty["ssim"].shape) == (0,) and tuple(empty["maps"].shape) == (0, h - 10, w - 10)
    call()                                                        # the unchanged arguments do run
    torch.cuda.synchronize()
    assert (score != SENTINEL).all() and (maps != SENTINEL).all()


def test_runs_on_the_callers_stream():
    from apnrf_amd import render as RD
    x, y, _ = _case(200, 160, 3)
    x, y = x.to(DEV), y.to(DEV)
    base = RD.ssim_views(x, y, maps=True)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(side):
        other = RD.ssim_views(x, y, maps=True)
    side.synchronize()
    assert torch.equal(_bits(other["ssim"]), _bits(base["ssim"])) and torch.equal(_bits(other["maps"]), _bits(base["maps"]))
    RD.release_workspaces(side)


def test_evaluate_views_with_ssim(scene, dataset):
    from apnrf_amd import render as RD
    field, est = H.hip_field(scene), H.hip_estimator(scene)
    h, w = dataset.height, dataset.width
    order = [2, 0, 1]
    with_ssim = RD.evaluate_views(field, est, dataset, order, views_per_call=2, return_images=True, ssim=True, **H.RENDER_KW)
    without = RD.evaluate_views(field, est, dataset, order, views_per_call=2, return_images=True, **H.RENDER_KW)
    today = {"rgb_mse", "psnr", "depth_mse", "sem_ce", "sem_acc", "confusion", "pixel_accuracy", "miou", "mean", "rgb", "acc", "depth", "sem"}
    assert set(without) == today and set(without["mean"]) == {"psnr", "depth_mse", "sem_ce"}
    assert set(with_ssim) == today | {"ssim"} and set(with_ssim["mean"]) == {"psnr", "depth_mse", "sem_ce", "ssim"}
    s = with_ssim["ssim"]
    assert isinstance(s, np.ndarray) and s.dtype == np.float64 and s.shape == (3,)
    assert with_ssim["mean"]["ssim"] == float(np.mean(s))
    assert torch.equal(with_ssim["rgb"].view(torch.int32), without["rgb"].view(torch.int32))
    direct = RD.ssim_metrics(with_ssim["rgb"], dataset, order)["ssim"].cpu().numpy()
    assert np.array_equal(s.view(np.int64), direct.view(np.int64))
    pixels = torch.stack([dataset[i]["pixels"] for i in order]).cpu().numpy()
    want = SR.ssim(with_ssim["rgb"].cpu().numpy(), pixels)[0]
    print("evaluate_views ssim", s, "restatement", want, "max abs diff", np.abs(s - want).max())
    np.testing.assert_allclose(s, want, rtol=RTOL, atol=ATOL)
    assert np.isfinite(s).all() and (np.abs(s) < 1.0).all()
    assert np.array_equal(with_ssim["psnr"].view(np.int64), without["psnr"].view(np.int64))
    assert np.array_equal(with_ssim["confusion"], without["confusion"])
    for name in ("rgb_mse", "depth_mse", "sem_ce", "sem_acc"):
        assert np.array_equal(with_ssim[name].view(np.int64), without[name].view(np.int64))
    plain = RD.evaluate_views(field, est, dataset, order, **H.RENDER_KW)          # the default call: no image keys either
    assert set(plain) == today - {"rgb", "acc", "depth", "sem"}
