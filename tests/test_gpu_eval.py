"""GPU tests of the held-out view evaluation: `mnf_eval_views` (csrc/eval.hip) through `render.eval_metrics`, and the whole
evaluation block `render.evaluate_views`.

The yardstick for the metrics is the reference's own expressions (scripts/pipeline.py:588-605: F.cross_entropy, F.mse_loss,
-10 log(mse) / log(10)) evaluated by torch in float64 on the CPU on the same fp32 values, with the ground truth gathered by the
existing `Dataset.__getitem__`; bar rtol 1e-9 / atol 1e-12, the bar `mnf_score_views` is held to against the float64 scorer: both
sides are double-precision reductions of the same fp32 inputs.  The confusion matrix and the label map must be equal exactly."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import helpers as H

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RTOL, ATOL = 1e-9, 1e-12
C = 29
N_IMAGES = 3


def _c2w(scene, n):
    from apnrf_amd import render as RD
    return np.stack([RD.pose_to_c2w(np.asarray(p, np.float64)) for p in scene["poses"][:n]]).astype(np.float32)


@pytest.fixture(scope="module")
def scene():
    return H.make_scene(log2_hashmap_size=15)


@pytest.fixture(scope="module")
def model(scene):
    return H.hip_field(scene), H.hip_estimator(scene)


def _make_datasets(scene, model, tmp, h, w, seed):
    """Two `Dataset(training=False)` (reference layout and packed) holding the same synthetic ground truth for N_IMAGES images of
    h x w pixels at the scene's first poses.  Labels: the model's own argmax on about half of the pixels, a uniformly random class on
    the others, so that the model is right on roughly half of them and wrong in many different cells of the matrix."""
    from apnrf_amd import render as RD
    from apnrf_amd.dataset import Dataset
    field, est = model
    rng = np.random.default_rng(seed)
    c2w = _c2w(scene, N_IMAGES)
    images = rng.integers(0, 256, size=(N_IMAGES, h, w, 3), dtype=np.uint8)
    depths = rng.uniform(0.2, 6.0, size=(N_IMAGES, h, w)).astype(np.float32)
    plain = Dataset(training=False, save_fp=str(tmp / f"plain{h}x{w}"), device=DEV)
    plain.update_data(images, depths, np.zeros((N_IMAGES, h, w), np.int64), c2w)       # labels follow: the rays come from this dataset
    sems = np.empty((N_IMAGES, h, w), np.int64)
    for i in range(N_IMAGES):
        _, _, _, sem, _ = RD.render_image_with_occgrid_test(1024, field, est, plain[i]["rays"], render_bkgd=torch.ones(3, device=DEV), **H.RENDER_KW)
        own = sem.argmax(-1).cpu().numpy()
        sems[i] = np.where(rng.random((h, w)) < 0.5, own, rng.integers(0, C, size=(h, w)))
    plain.semantics = torch.from_numpy(sems).to(DEV)
    packed = Dataset(training=False, save_fp=str(tmp / f"packed{h}x{w}"), device=DEV, packed=True)
    packed.update_data(images, depths, sems, c2w)
    assert packed.depths.dtype == torch.float16 and packed.semantics.dtype == torch.uint8 and plain.semantics.dtype == torch.int64
    return {"plain": plain, "packed": packed}


@pytest.fixture(scope="module")
def small(scene, model, tmp_path_factory):
    return _make_datasets(scene, model, tmp_path_factory.mktemp("eval_small"), 48, 40, 1)          # non-square: H = 48, W = 40


@pytest.fixture(scope="module")
def large(scene, model, tmp_path_factory):
    return _make_datasets(scene, model, tmp_path_factory.mktemp("eval_large"), 200, 160, 2)        # 32000 pixels: many workgroups per view


def _random_renders(V, P, seed):
    g = torch.Generator().manual_seed(seed)
    rgb = torch.rand(V, P, 3, generator=g)
    depth = torch.rand(V, P, generator=g) * 6.0
    sem = torch.randn(V, P, C, generator=g) * 3.0
    return rgb, depth, sem


def _torch_f64(rgb, depth, sem, ds, image_ids, pix):
    """The reference's expressions in float64 on the CPU; ground truth through `Dataset.__getitem__`.  rgb [V,P,3], depth [V,P],
    sem [V,P,C] CPU fp32; pix: LongTensor [P] of flat pixel indices (row-major).  -> metrics [V,8], confusion [C,C], labels [V,P]"""
    V, P, Cn = sem.shape
    met = np.zeros((V, 8))
    conf = np.zeros((Cn, Cn), np.int64)
    pred_all = np.zeros((V, P), np.uint8)
    for k, i in enumerate(image_ids):
        data = ds[int(i)]
        pixels = data["pixels"].cpu().reshape(-1, 3)[pix].double()
        dep = data["dep"].cpu().reshape(-1)[pix].double()
        gt = data["sem"].cpu().reshape(-1)[pix]
        ok = (gt >= 0) & (gt < Cn)
        mse = F.mse_loss(rgb[k].double(), pixels)
        met[k, 0] = mse.item()
        met[k, 1] = (-10.0 * torch.log(mse) / np.log(10.0)).item()
        met[k, 2] = F.mse_loss(depth[k].double(), dep).item()
        pred = sem[k].double().argmax(-1)
        if ok.any():
            met[k, 3] = F.cross_entropy(sem[k].double()[ok], gt[ok]).item()
            met[k, 4] = (pred[ok] == gt[ok]).double().mean().item()
        else:
            met[k, 3] = met[k, 4] = np.nan
        met[k, 5], met[k, 6] = int(ok.sum()), int((~ok).sum())
        np.add.at(conf, (gt[ok].numpy(), pred[ok].numpy()), 1)
        pred_all[k] = pred.numpy().astype(np.uint8)
    return met, conf, pred_all


def _check(got, want_met, want_conf, want_pred, what):
    met = got["metrics"].cpu().numpy()
    for k, name in enumerate(("rgb_mse", "psnr", "depth_mse", "sem_ce", "sem_acc", "n_valid", "n_invalid", "reserved")):
        err = np.abs(met[:, k] - want_met[:, k])
        print(f"{what} {name}: got {met[:, k]} want {want_met[:, k]} max abs diff {np.nanmax(err) if err.size else 0:.3e}")
    np.testing.assert_allclose(met, want_met, rtol=RTOL, atol=ATOL, err_msg=what)
    np.testing.assert_array_equal(got["confusion"].cpu().numpy(), want_conf, err_msg=what)
    np.testing.assert_array_equal(got["pred_labels"].cpu().numpy(), want_pred, err_msg=what)


def test_fixture_is_not_vacuous(model, small, large):
    """The model must be partly right and partly wrong on the synthetic labels, or accuracy and the matrix test nothing."""
    from apnrf_amd import render as RD
    field, est = model
    for dss in (small, large):
        ds = dss["plain"]
        r = RD.evaluate_views(field, est, ds, [0, 1, 2], **H.RENDER_KW)
        acc = r["pixel_accuracy"]
        off_diagonal = int(r["confusion"].sum() - np.trace(r["confusion"]))
        print(f"fixture {ds.height}x{ds.width}: pixel accuracy {acc:.4f}, off-diagonal count {off_diagonal}, per-view {r['sem_acc']}")
        assert 0.2 < acc < 0.8
        assert all(0.2 < a < 0.8 for a in r["sem_acc"])
        assert off_diagonal > 0 and np.trace(r["confusion"]) > 0
        assert r["confusion"].sum() == 3 * ds.height * ds.width


@pytest.mark.parametrize("layout", ["plain", "packed"])
@pytest.mark.parametrize("case", ["48x40", "200x160", "P1", "P63", "ids_2_0_2", "pix_idx"])
def test_kernel_matches_torch_float64(small, large, layout, case):
    """`eval_metrics` on random renders against torch float64 on the CPU.  The packed dataset hands out fp16-rounded depths through
    `__getitem__` (as test_dataset_matches_reference checks), which is what the kernel must compare against."""
    from apnrf_amd import render as RD
    ds = (large if case == "200x160" else small)[layout]
    ppi = ds.height * ds.width
    rng = np.random.default_rng(7)
    image_ids, pix, explicit = [0, 1], torch.arange(ppi), False
    if case == "P1":
        pix, explicit = torch.tensor([ppi - 1]), True
    elif case == "P63":
        pix, explicit = torch.from_numpy(rng.choice(ppi, size=63, replace=False)), True
    elif case == "ids_2_0_2":
        image_ids = [2, 0, 2]
    elif case == "pix_idx":
        pix, explicit = torch.from_numpy(rng.permutation(ppi)[: ppi - 5]), True           # shuffled, not all pixels, P % 4 != 0
    elif case == "200x160":
        image_ids = [1, 2, 0]                                                              # odd V * P * C offsets: unaligned row starts
    P = int(pix.shape[0])
    rgb, depth, sem = _random_renders(len(image_ids), P, 11)
    got = RD.eval_metrics(rgb.to(DEV), depth.to(DEV), sem.to(DEV), ds, image_ids, pix_idx=pix.to(DEV) if explicit else None,
                          confusion=True, labels=True)
    assert got["metrics"].is_cuda and got["metrics"].dtype == torch.float64 and got["confusion"].dtype == torch.int64
    assert got["pred_labels"].dtype == torch.uint8 and tuple(got["pred_labels"].shape) == (len(image_ids), P)
    want = _torch_f64(rgb, depth, sem, ds, image_ids, pix)
    _check(got, *want, what=f"{layout} {case}")
    assert (want[0][:, 6] == 0).all() and got["confusion"].sum().item() == len(image_ids) * P
    if case == "48x40":       # the [V,H,W,...] forms and host-side pix_idx are the same call; optional outputs can be left out
        again = RD.eval_metrics(rgb.view(2, 48, 40, 3).to(DEV), depth.view(2, 48, 40, 1).to(DEV), sem.view(2, 48, 40, C).to(DEV), ds,
                                torch.tensor(image_ids), pix_idx=np.arange(ppi), confusion=False, labels=False)
        assert again["confusion"] is None and again["pred_labels"] is None
        assert torch.equal(again["metrics"], got["metrics"])


def test_even_class_count_and_more_than_64_classes(small):
    """C = 12 takes the padded LDS rows (row stride C | 1), C = 70 counts the matrix with global atomics (no LDS histogram)."""
    from apnrf_amd import render as RD
    ds = small["plain"]
    ppi = ds.height * ds.width
    for Cn in (12, 70):
        g = torch.Generator().manual_seed(Cn)
        rgb, depth = torch.rand(2, ppi, 3, generator=g), torch.rand(2, ppi, generator=g)
        sem = torch.randn(2, ppi, Cn, generator=g)
        got = RD.eval_metrics(rgb.to(DEV), depth.to(DEV), sem.to(DEV), ds, [1, 2], confusion=True, labels=True)
        want = _torch_f64(rgb, depth, sem, ds, [1, 2], torch.arange(ppi))
        _check(got, *want, what=f"C={Cn}")
        if Cn == 12:
            assert want[0][0, 6] > 0          # labels 12..28 of the fixture are outside [0, 12): counted, not scored


def test_ties_predict_the_lower_index(small):
    from apnrf_amd import render as RD
    ds = small["plain"]
    ppi = ds.height * ds.width
    rgb, depth, sem = _random_renders(1, ppi, 5)
    sem[0, 10, :] = -1.0; sem[0, 10, 7] = 4.0; sem[0, 10, 19] = 4.0           # two equal maxima
    sem[0, 11, :] = 2.5                                                      # all equal
    sem[0, 12, :] = -3.0; sem[0, 12, 28] = 0.5; sem[0, 12, 0] = 0.5
    got = RD.eval_metrics(rgb.to(DEV), depth.to(DEV), sem.to(DEV), ds, [1], labels=True)
    pred = got["pred_labels"].cpu().numpy()[0]
    assert pred[10] == 7 and pred[11] == 0 and pred[12] == 0
    _check(got, *_torch_f64(rgb, depth, sem, ds, [1], torch.arange(ppi)), what="ties")


def test_labels_outside_the_classes_are_counted_and_refused(model, small, scene, tmp_path):
    from apnrf_amd import render as RD
    from apnrf_amd.dataset import Dataset
    field, est = model
    src = small["plain"]
    h, w = src.height, src.width
    sems = src.semantics.cpu().numpy().copy()
    sems[1, 3, :17] = C               # just past the last class
    sems[1, 20, 5] = 255
    sems[1, 21, 6] = -1               # int64 storage can hold a negative id
    bad = Dataset(training=False, save_fp=str(tmp_path / "bad"), device=DEV)
    bad.update_data(src.images.cpu().numpy(), src.depths.cpu().numpy(), sems, src.camtoworlds.cpu().numpy())
    rgb, depth, sem = _random_renders(2, h * w, 3)
    got = RD.eval_metrics(rgb.to(DEV), depth.to(DEV), sem.to(DEV), bad, [0, 1], labels=True)
    met = got["metrics"].cpu().numpy()
    assert met[0, 6] == 0 and met[0, 5] == h * w
    assert met[1, 6] == 19 and met[1, 5] == h * w - 19
    assert got["confusion"].sum().item() == 2 * h * w - 19
    _check(got, *_torch_f64(rgb, depth, sem, bad, [0, 1], torch.arange(h * w)), what="bad labels")      # columns 3-5 over the valid pixels only
    with pytest.raises(ValueError, match="outside"):
        RD.evaluate_views(field, est, bad, [0, 1], **H.RENDER_KW)
    assert RD.evaluate_views(field, est, bad, [0, 2], **H.RENDER_KW)["psnr"].shape == (2,)               # the clean images still evaluate


def test_nan_stays_in_its_view_and_its_columns(small):
    from apnrf_amd import render as RD
    ds = small["packed"]
    ppi = ds.height * ds.width
    rgb, depth, sem = _random_renders(3, ppi, 9)
    clean = RD.eval_metrics(rgb.to(DEV), depth.to(DEV), sem.to(DEV), ds, [0, 1, 2])["metrics"].cpu().numpy()
    rgb[1, 1234, 2] = float("nan")
    met = RD.eval_metrics(rgb.to(DEV), depth.to(DEV), sem.to(DEV), ds, [0, 1, 2])["metrics"].cpu().numpy()
    assert np.isnan(met[1, 0]) and np.isnan(met[1, 1])
    assert np.isfinite(met[1, 2:]).all() and np.isfinite(met[[0, 2]]).all()
    np.testing.assert_array_equal(met[[0, 2]], clean[[0, 2]])
    np.testing.assert_array_equal(met[1, 2:], clean[1, 2:])


def test_two_runs_are_bitwise_equal(large):
    from apnrf_amd import render as RD
    ds = large["plain"]
    rgb, depth, sem = (t.to(DEV) for t in _random_renders(3, ds.height * ds.width, 21))
    a = RD.eval_metrics(rgb, depth, sem, ds, [0, 1, 2], labels=True)
    b = RD.eval_metrics(rgb, depth, sem, ds, [0, 1, 2], labels=True)
    assert torch.equal(a["metrics"].view(torch.int64), b["metrics"].view(torch.int64))
    assert torch.equal(a["confusion"], b["confusion"]) and torch.equal(a["pred_labels"], b["pred_labels"])
    # a view's row does not depend on the other views of the call either
    alone = RD.eval_metrics(rgb[1:2], depth[1:2], sem[1:2], ds, [1])
    assert torch.equal(alone["metrics"].view(torch.int64)[0], a["metrics"].view(torch.int64)[1])


@pytest.mark.parametrize("V,P,Cn", [(3, 301, 29),      # unpadded LDS rows, two tiles per view, odd view starts
                                    (2, 63, 64)])       # padded rows (row stride C | 1 != C), one short tile
def test_inputs_off_the_16_byte_grid(small, V, P, Cn):
    """rgb, depth and sem starting 1, 2 and 3 floats into larger allocations (contiguous views of a flat buffer, which `eval_metrics` passes
    through as they are: the staging takes a scalar head up to the first 16-byte boundary of the address) give the bits of the same values in
    tensors of their own."""
    from apnrf_amd import render as RD
    ds = small["plain"]
    g = torch.Generator().manual_seed(100 + Cn)
    own = [torch.rand(V, P, 3, generator=g).to(DEV), (torch.rand(V, P, generator=g) * 6.0).to(DEV), (torch.randn(V, P, Cn, generator=g) * 3.0).to(DEV)]
    shifted = []
    for off, t in zip((1, 2, 3), own):
        flat = torch.empty(t.numel() + 8, device=DEV)
        view = flat[off:off + t.numel()].view(t.shape)
        view.copy_(t)
        assert view.is_contiguous() and t.data_ptr() % 16 == 0 and view.data_ptr() % 16 == 4 * off
        shifted.append(view)
    want = RD.eval_metrics(*own, ds, list(range(V)), labels=True)
    got = RD.eval_metrics(*shifted, ds, list(range(V)), labels=True)
    assert np.isfinite(want["metrics"].cpu().numpy()).all() and want["confusion"].sum().item() == V * P
    assert torch.equal(got["metrics"].view(torch.int64), want["metrics"].view(torch.int64))
    assert torch.equal(got["confusion"], want["confusion"]) and torch.equal(got["pred_labels"], want["pred_labels"])


def test_evaluate_views_end_to_end(model, small):
    from apnrf_amd import render as RD
    field, est = model
    ds = small["plain"]
    h, w = ds.height, ds.width
    order = [2, 0, 1]
    r = RD.evaluate_views(field, est, ds, order, views_per_call=2, return_images=True, labels=True, **H.RENDER_KW)
    assert tuple(r["rgb"].shape) == (3, h, w, 3) and tuple(r["sem"].shape) == (3, h, w, C) and tuple(r["pred_labels"].shape) == (3, h, w)
    for k, i in enumerate(order):       # the per-image call a user of the import swap makes today
        data = ds[i]
        rgb, acc, depth, sem, _ = RD.render_image_with_occgrid_test(1024, field, est, data["rays"], render_bkgd=data["color_bkgd"], **H.RENDER_KW)
        for name, one in (("rgb", rgb), ("acc", acc), ("depth", depth), ("sem", sem)):
            assert r[name][k].shape == one.shape
            assert torch.equal(r[name][k].view(torch.int32), one.view(torch.int32)), f"{name} of image {i} differs from the per-image render"
    P = h * w
    want_met, want_conf, want_pred = _torch_f64(r["rgb"].cpu().view(3, P, 3), r["depth"].cpu().view(3, P), r["sem"].cpu().view(3, P, C), ds, order,
                                                torch.arange(P))
    got = np.stack([r["rgb_mse"], r["psnr"], r["depth_mse"], r["sem_ce"], r["sem_acc"]], axis=1)
    print("evaluate_views metrics", got, "torch float64", want_met[:, :5])
    np.testing.assert_allclose(got, want_met[:, :5], rtol=RTOL, atol=ATOL)
    for name in ("rgb_mse", "psnr", "depth_mse", "sem_ce", "sem_acc"):
        assert r[name].dtype == np.float64 and r[name].shape == (3,)
    np.testing.assert_array_equal(r["confusion"], want_conf)
    assert r["confusion"].dtype == np.int64
    np.testing.assert_array_equal(r["pred_labels"].cpu().numpy().reshape(3, P), want_pred)
    assert r["mean"] == {"psnr": float(np.mean(r["psnr"])), "depth_mse": float(np.mean(r["depth_mse"])), "sem_ce": float(np.mean(r["sem_ce"]))}
    assert r["miou"] == RD.miou_from_confusion(r["confusion"]) and 0.0 < r["miou"] < 1.0
    assert r["pixel_accuracy"] == np.trace(want_conf) / want_conf.sum()
    # grouping and storage layout change nothing
    r4 = RD.evaluate_views(field, est, small["packed"], order, views_per_call=4, **H.RENDER_KW)
    np.testing.assert_array_equal(r4["confusion"], r["confusion"])
    for name in ("rgb_mse", "psnr", "sem_ce", "sem_acc"):
        np.testing.assert_array_equal(r4[name], r[name])
    assert "rgb" not in r4 and "pred_labels" not in r4


def test_runs_on_the_callers_stream_without_synchronising(large):
    from apnrf_amd import render as RD
    ds = large["packed"]
    rgb, depth, sem = (t.to(DEV) for t in _random_renders(2, ds.height * ds.width, 4))
    base = RD.eval_metrics(rgb, depth, sem, ds, [2, 1], labels=True)
    assert all(base[k].is_cuda for k in ("metrics", "confusion", "pred_labels"))
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(side):
        other = RD.eval_metrics(rgb, depth, sem, ds, [2, 1], labels=True)
    side.synchronize()
    assert torch.equal(other["metrics"].view(torch.int64), base["metrics"].view(torch.int64))
    assert torch.equal(other["confusion"], base["confusion"]) and torch.equal(other["pred_labels"], base["pred_labels"])
    RD.release_workspaces(side)
