"""GPU tests of the 8-bit frame conversion: `mnf_frames_views` (csrc/frames.hip) through `render.frames_from_renders` and through the raw
entry point, and the whole route `render.render_frames`.

The yardstick is tests/frames_ref.py: the reference's host expressions (scripts/pipeline.py:994-1022, the viewer's depth form) in numpy
on float64, then rint of the clipped value.  Outputs are integers and the arithmetic is fully specified, so every comparison is exact
equality: there is no tolerance."""

import numpy as np
import pytest
import torch

import frames_ref as FR
import helpers as H

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN, INF = float("nan"), float("inf")
GUARD = 0xA5
# (V, P, C, K): one pixel; odd P (views 1 and 2 start off the 16-byte and 4-byte grids) with the reference's 29 classes and 40 colours; an
# even class count (padded LDS rows) with P = 257: two tiles, the second of one pixel; C = 33: rows longer than a wave's 32 banks;
# C = 256: the largest count with a label plane, tiles of 36 pixels
SHAPES = [(1, 1, 1, 1), (3, 185, 29, 40), (2, 257, 32, 32), (2, 64, 33, 40), (1, 300, 256, 256)]


def _fill(flat, values):
    n = min(flat.size, values.size)
    flat[:n] = values[:n]


def make_planes(V, P, C, K, seed):
    """Seeded random planes holding the boundary sets (as far as they fit: all of them at V * P >= 513), NaN and both infinities, and
    logit rows with ties, NaN and an all -inf row."""
    rng = np.random.default_rng(seed)
    n = V * P
    rgb = rng.uniform(-0.1, 1.2, (n, 3)).astype(np.float32)
    acc = rng.uniform(-0.1, 1.2, n).astype(np.float32)
    depth = rng.uniform(-1.0, 14.0, n).astype(np.float32)
    sem = (rng.standard_normal((n, C)) * 3.0).astype(np.float32)
    unit, dep = FR.unit_boundary_set(), FR.depth_boundary_set()
    _fill(rgb.reshape(-1), np.concatenate([unit, unit[::-1], unit]))
    _fill(acc, unit)
    _fill(depth, dep)
    special = np.float32([NAN, INF, -INF])
    for plane in (rgb.reshape(-1), acc, depth):
        if plane.size >= 3:
            plane[-3:] = special
        else:
            plane[-1] = NAN
    if C >= 2:
        tie = np.full(C, -1.0, np.float32); tie[C // 3] = 4.0; tie[C - 1] = 4.0
        nan1 = rng.standard_normal(C).astype(np.float32); nan1[C // 2] = NAN
        nan2 = rng.standard_normal(C).astype(np.float32); nan2[C - 1] = NAN; nan2[1] = NAN; nan2[0] = 50.0
        rows = [tie, np.full(C, 2.5, np.float32), nan1, nan2, np.full(C, -INF, np.float32)]
    else:
        rows = [np.float32([NAN])]
    for k, row in enumerate(rows):
        for at in (k, n - 1 - k):                        # in the first tile of the first view and in the last tile of the last
            if 0 <= at < n:
                sem[at] = row
    palette = rng.integers(0, 256, (K, 3), dtype=np.uint8)
    return rgb.reshape(V, P, 3), depth.reshape(V, P), acc.reshape(V, P), sem.reshape(V, P, C), palette


def _assert_planes(got, want, what, labels):
    for name in ("rgb", "depth", "occ", "sem") + (("labels",) if labels else ()):
        g = got[name].cpu().numpy() if isinstance(got[name], torch.Tensor) else got[name]
        w = want[name].astype(np.uint8)
        assert g.dtype == np.uint8 and g.shape == w.shape, (what, name, g.dtype, g.shape, w.shape)
        bad = np.argwhere(g != w)
        assert bad.size == 0, f"{what}: plane {name} differs at {len(bad)} places, first {bad[0].tolist()}: got {g[tuple(bad[0])]} want {w[tuple(bad[0])]}"


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "V{}_P{}_C{}_K{}".format(*s))
def test_kernel_matches_restatement(shape):
    from apnrf_amd import render as RD
    V, P, C, K = shape
    rgb, depth, acc, sem, palette = make_planes(V, P, C, K, seed=P + C)
    if V * P >= 513:
        assert (FR.depth_f32_form(depth) != FR.dep8(depth)).any() and (FR.rgb_f64_form(rgb) != FR.rgb8(rgb)).any()     # the inputs tell the precisions apart
    dev = [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in (rgb, depth, acc, sem)]
    for depth_map, ref_map in ((RD.FRAME_DEPTH_PIPELINE, FR.DEPTH_PIPELINE), (RD.FRAME_DEPTH_VIEWER, FR.DEPTH_VIEWER)):
        for order in ("bgr", "rgb"):
            want = FR.frames(rgb, depth, acc, sem, palette, ref_map, order)
            for labels in (True, False):
                got = RD.frames_from_renders(*dev, palette, depth_map=depth_map, channel_order=order, labels=labels)
                assert ("labels" in got) == labels and all(t.is_cuda and t.dtype == torch.uint8 for t in got.values())
                _assert_planes(got, want, f"{shape} {ref_map} {order} labels={labels}", labels)
    # the [V,H,W,...] forms with [V,H,W,1] depth and acc, a device palette tensor and a depth map of the caller's
    if P == 300:
        d4 = [dev[0].view(V, 15, 20, 3), dev[1].view(V, 15, 20, 1), dev[2].view(V, 15, 20, 1), dev[3].view(V, 15, 20, C)]
        own = (2.0, 4.0, 3.0, 10.0)
        got = RD.frames_from_renders(*d4, torch.from_numpy(palette).to(DEV), depth_map=own, labels=True)
        want = FR.frames(rgb, depth, acc, sem, palette, own, "bgr")
        assert tuple(got["rgb"].shape) == (V, 15, 20, 3) and tuple(got["depth"].shape) == (V, 15, 20) and tuple(got["labels"].shape) == (V, 15, 20)
        _assert_planes({k: t.reshape(want[k].shape) for k, t in got.items()}, want, f"{shape} 4-d forms", True)


def test_label_plane_needs_at_most_256_classes():
    from apnrf_amd import render as RD
    V, P, C = 1, 40, 300
    rgb, depth, acc, sem, palette = make_planes(V, P, C, C, seed=3)
    dev = [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in (rgb, depth, acc, sem)]
    with pytest.raises(ValueError, match="256"):
        RD.frames_from_renders(*dev, palette, labels=True)
    with pytest.raises(ValueError, match="colours"):
        RD.frames_from_renders(*dev, palette[:299])
    with pytest.raises(ValueError, match="channel_order"):
        RD.frames_from_renders(*dev, palette, channel_order="gbr")
    # without the label plane 300 classes are fine: the colour plane holds palette entries, not class ids
    got = RD.frames_from_renders(*dev, palette)
    _assert_planes(got, FR.frames(rgb, depth, acc, sem, palette), "C=300", False)


def _dev_ptr(addr):
    from apnrf_amd import _lib as L
    p = L.DevPtr(addr)
    p.device = torch.device(DEV)
    return p


@pytest.mark.parametrize("off", [1, 2, 3])
def test_unaligned_inputs_and_guarded_outputs(off):
    """The raw entry point: `sem` 4 bytes into its allocation (a scalar head of three floats, then 16-byte loads, then a scalar tail), rgb / depth / acc 4 bytes in as
    well, every output `off` bytes into a buffer pre-filled with 0xA5.  Results equal the restatement and no guard byte changes."""
    from apnrf_amd import _lib as L
    lib = L.load_library()
    V, P, C, K = 3, 185, 29, 40
    rgb, depth, acc, sem, palette = make_planes(V, P, C, K, seed=17 + off)
    ins = []
    for a in (rgb, depth, acc, sem):
        big = torch.empty(a.size + 1, dtype=torch.float32, device=DEV)
        big[1:] = torch.from_numpy(a.reshape(-1)).to(DEV)
        assert (big.data_ptr() + 4) % 16 == 4
        ins.append(big)
    pal = torch.from_numpy(palette).to(DEV)
    pad = 64
    sizes = dict(rgb=V * P * 3, depth=V * P, occ=V * P, sem=V * P * 3, labels=V * P)
    bufs = {k: torch.full((pad + off + n + pad,), GUARD, dtype=torch.uint8, device=DEV) for k, n in sizes.items()}
    outs = {k: _dev_ptr(b.data_ptr() + pad + off) for k, b in bufs.items()}
    assert all(b.data_ptr() % 4 == 0 for b in bufs.values())
    L.launch(lib.mnf_frames_views, *[_dev_ptr(t.data_ptr() + 4) for t in ins], V, P, C, L.ptr(pal), K, *FR.DEPTH_PIPELINE, 1,
             outs["rgb"], outs["depth"], outs["occ"], outs["sem"], outs["labels"])
    want = FR.frames(rgb, depth, acc, sem, palette, FR.DEPTH_PIPELINE, "bgr")
    for k, n in sizes.items():
        host = bufs[k].cpu().numpy()
        assert (host[:pad + off] == GUARD).all(), f"{k}: a byte before the output was written (offset {off})"
        assert (host[pad + off + n:] == GUARD).all(), f"{k}: a byte after the output was written (offset {off})"
        np.testing.assert_array_equal(host[pad + off:pad + off + n], want[k].astype(np.uint8).reshape(-1), err_msg=f"{k} at offset {off}")
    # skipped outputs stay untouched: only the depth plane is asked for, and sem / palette may then be null
    for b in bufs.values():
        b.fill_(GUARD)
    L.launch(lib.mnf_frames_views, None, _dev_ptr(ins[1].data_ptr() + 4), None, None, V, P, C, None, 0, *FR.DEPTH_VIEWER, 0, None, outs["depth"], None,
             None, None)
    host = {k: b.cpu().numpy() for k, b in bufs.items()}
    np.testing.assert_array_equal(host["depth"][pad + off:pad + off + V * P], FR.dep8(depth, FR.DEPTH_VIEWER).reshape(-1))
    assert all((host[k] == GUARD).all() for k in ("rgb", "occ", "sem", "labels"))
    assert (host["depth"][:pad + off] == GUARD).all() and (host["depth"][pad + off + V * P:] == GUARD).all()


# ------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def scene():
    return H.make_scene(log2_hashmap_size=15)


@pytest.fixture(scope="module")
def model(scene):
    return H.hip_field(scene), H.hip_estimator(scene)


@pytest.mark.parametrize("width, height, scale", [(24, 20, 1), (48, 40, 0.5)])
def test_render_frames_end_to_end(scene, model, width, height, scale):
    """`render_frames` against the parent route: the restatement applied to `render_image_from_pose`'s float64 stacks, byte for byte."""
    from apnrf_amd import render as RD
    field, est = model
    poses = scene["poses"][:3]
    focal = 0.5 * width / np.tan(np.pi / 4)
    kw = H.RENDER_KW
    args = (field, est, poses, width, height, focal, kw["near_plane"], kw["render_step_size"], scale, kw["cone_angle"], kw["alpha_thre"])
    images, depths, accs, sems = RD.render_image_from_pose(*args, None, DEV)
    h, w = int(height * scale), int(width * scale)
    assert images.shape == (3, h, w, 3) and sems.shape == (3, h, w, 29)
    assert images.max() > 0.05 and accs.max() > 0.5 and len(np.unique(np.argmax(sems, -1))) > 1       # not an empty render
    palette = np.random.default_rng(5).integers(0, 256, (40, 3), dtype=np.uint8)
    want = FR.frames(images, depths, accs, sems, palette, FR.DEPTH_PIPELINE, "bgr")
    base = None
    for per in (1, 2, 4):
        got = RD.render_frames(*args, palette, labels=True, views_per_call=per, device=DEV)
        assert all(isinstance(a, np.ndarray) for a in got.values())
        _assert_planes(got, want, f"{width}x{height} views_per_call={per}", True)
        base = base or got
        assert all(np.array_equal(got[k], base[k]) for k in got)
    on_dev = RD.render_frames(*args, palette, labels=True, to_host=False, device=DEV)
    assert all(t.is_cuda and t.dtype == torch.uint8 for t in on_dev.values())
    _assert_planes(on_dev, want, "to_host=False", True)
    # the viewer's mapping, RGB order, no label plane
    view = RD.render_frames(*args, palette, depth_map=RD.FRAME_DEPTH_VIEWER, channel_order="rgb", device=DEV)
    assert "labels" not in view
    _assert_planes(view, FR.frames(images, depths, accs, sems, palette, FR.DEPTH_VIEWER, "rgb"), "viewer", False)
