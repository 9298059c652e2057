"""GPU tests of TSDF fusion (csrc/tsdf.hip, mnf_surface_extract_observed in csrc/surface.hip, apnrf_amd/tsdf.py) against the numpy
restatement tests/tsdf_ref.py, which tests/test_tsdf_cpu.py holds to the definition.  Every call goes through the C ABI with canaries on
both sides of every output, twice, and the two runs must give the same bytes.

The lattice is 21 x 10 x 22 points (the room's 20 x 10 x 22 widened by one cell in x): none of the block shapes the unit can be built with
(4 x 4 x 16, 1 x 4 x 64, 2 x 8 x 16) divides it on any axis, and each spans several blocks on at least two axes.  The seven views are the
room's: four at the centre (the camera is inside the volume, with points behind it), one that misses the volume, two repeats; view 1
holds planted NaN, inf, 0 and over-range depths, and the int64 layout a class of 300.

In planar mode everything is `array_equal` to the restatement: both sides round every float64 operation separately and in the same order,
and IEEE division is correctly rounded on both.  In ray mode `along` is a float64 square root; the device's is assumed correctly rounded,
not bit-equal to numpy's (as tests/test_gpu_sensor.py assumes of the sensor's), so `tsdf` and `best` are held to one float32 ulp there and
weight, word and info to the byte; the test prints whether the bytes were equal after all (on one MI355X they were, in both layouts).

The second group leaves the yaw poses: 24 general poses (no rotation entry is 0 or 1, so every index of the point chain and of the block
cull matters), the same under a skew (the cull's bound needs the column norms), min_depth and max_depth that bind, three degenerate poses,
and a list of 600 views (more than one wave of survivors per block, a second and a third chunk, a block first reached in the second chunk
and one never reached, views that tie in |sdf| across waves).  tests/test_tsdf_cpu.py shows that these inputs reach those cases."""
import ctypes

import numpy as np
import pytest
import torch

import sensor_ref as SR
import surface_ref as SF
import tsdf_ref as T

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CANARY = 64
MARKS = {torch.uint8: 0xA5, torch.int32: -0x5A5A5A5B, torch.int64: -0x5A5A5A5A5A5A5A5B, torch.float32: -12345.5}
CELLS = (20, 9, 21)
S, TRUNC = T.S, 4 * T.S


def _dev(a):
    return torch.from_numpy(np.array(a, copy=True, order="C")).to(DEV)


def _guarded(n, dtype):
    whole = torch.full((n + 2 * CANARY,), MARKS[dtype], dtype=dtype, device=DEV)
    return whole, whole[CANARY:CANARY + n]


def _assert_guards(whole, n, what):
    host, mark = whole.cpu().numpy(), MARKS[whole.dtype]
    assert (host[:CANARY] == mark).all() and (host[CANARY + n:] == mark).all(), f"{what}: written outside its bounds"


def _lib():
    from apnrf_amd import _lib as L
    return L, L.load_library()


def _c3(v):
    return (ctypes.c_double * 3)(*[float(x) for x in v])


_CAPTURES = {}


def captures(mode, layout):
    """-> (c2w, depth, colour, classes) as numpy arrays in storage layout "wide" (RGBA / f32 / i64 with a patch of class 300) or "packed"
    (RGB / f16 / u8)."""
    if (mode, layout) not in _CAPTURES:
        c2w, depth, rgba, sem = T.room_captures(mode, repeats=2)
        if layout == "wide":
            sem = sem.astype(np.int64)
            sem[0, 4:12, 6:18] = 300
            sem[2, 0, 0] = -1
            out = (c2w, depth, rgba, sem)
        else:
            out = (c2w, depth.astype(np.float16), np.ascontiguousarray(rgba[..., :3]), sem)
        for a in out:
            a.setflags(write=False)
        _CAPTURES[(mode, layout)] = out
    return _CAPTURES[(mode, layout)]


def fresh(max_weight=64):
    return T.Volume(CELLS, T.ROOM_LO, S, TRUNC, max_weight=max_weight)


def gpu_integrate(vol, c2w, depth, colour, classes, mode, one_by_one=False, calls=None):
    """mnf_tsdf_integrate on a copy of `vol`'s state -> a Volume holding what the device left.  Twice; the same bytes both times.  `calls`
    is a list of view counts, one call each, in order (all views in one call when None)."""
    L, lib = _lib()
    n = int(np.prod(vol.shape))
    V, H, W = depth.shape
    d_m, d_d, d_c, d_k = _dev(np.asarray(c2w, np.float64).reshape(-1, 3, 4)), _dev(depth), _dev(colour), _dev(classes)
    outs = []
    for _ in range(2):
        bufs = [_guarded(n, torch.float32), _guarded(n, torch.int32), _guarded(n, torch.int32), _guarded(n, torch.float32), _guarded(5, torch.int64)]
        for (whole, part), init in zip(bufs, (vol.tsdf, vol.weight, vol.word.view(np.int32), vol.best, vol.info)):
            part.copy_(_dev(init.reshape(-1)))
        t, w, wd, b, info = (p for _, p in bufs)
        ends = np.cumsum([1] * V if one_by_one else [V] if calls is None else calls).tolist()
        assert ends[-1:] == [V] or V == 0
        for lo_v, hi_v in zip([0] + ends[:-1], ends):
            L.launch(lib.mnf_tsdf_integrate, L.ptr(t), L.ptr(w), L.ptr(wd), L.ptr(b), *vol.cells, _c3(vol.lo), float(vol.voxel), float(vol.trunc), vol.max_weight,
                     float(vol.min_depth), float(vol.max_depth), L.ptr(d_m[lo_v:hi_v]), hi_v - lo_v, W, H, T.FOCAL, L.ptr(d_d[lo_v:hi_v]),
                     1 if depth.dtype == np.float16 else 0, L.ptr(d_c[lo_v:hi_v]), colour.shape[-1], L.ptr(d_k[lo_v:hi_v]), 1 if classes.dtype == np.int64 else 0,
                     mode, L.ptr(info), device=torch.device(DEV))
        torch.cuda.synchronize()
        for (whole, _), k, what in zip(bufs, (n, n, n, n, 5), ("tsdf", "weight", "word", "best", "info")):
            _assert_guards(whole, k, what)
        got = vol.copy()
        got.tsdf, got.weight, got.best = (x.cpu().numpy().reshape(vol.shape) for x in (t, w, b))
        got.word, got.info = wd.cpu().numpy().view(np.uint32).reshape(vol.shape), info.cpu().numpy()
        outs.append(got)
    for k in ("tsdf", "weight", "word", "best", "info"):
        assert getattr(outs[0], k).tobytes() == getattr(outs[1], k).tobytes(), f"{k} differs between two runs"
    return outs[0]


def _same_bits(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def _within_one_ulp(got, want):
    return bool(((got == want) | (np.abs(got.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want)))).all())


# ------------------------------------------------------------------ fusion against the restatement
@pytest.mark.parametrize("layout", ["wide", "packed"])
@pytest.mark.parametrize("mode", [T.PLANAR, T.RAY])
def test_integrate_equals_the_restatement(mode, layout):
    c2w, depth, colour, classes = captures(mode, layout)
    want = T.integrate(fresh(3), c2w, T.FOCAL, depth, colour, classes, mode)
    got = gpu_integrate(fresh(3), c2w, depth, colour, classes, mode)
    assert want.info[0] > 3000 and want.info[2] > 0 and want.info[3] > 0 and (want.weight == 3).any() and want.info[0] > want.weight.sum()
    assert (want.info[4] > 0) == (layout == "wide")
    np.testing.assert_array_equal(got.weight, want.weight)
    np.testing.assert_array_equal(got.word, want.word)
    np.testing.assert_array_equal(got.info, want.info)
    if mode == T.PLANAR:
        assert _same_bits(got.tsdf, want.tsdf) and _same_bits(got.best, want.best)
    else:
        print(f"ray mode, {layout}: tsdf bytes equal {_same_bits(got.tsdf, want.tsdf)}, best bytes equal {_same_bits(got.best, want.best)}")
        assert _within_one_ulp(got.tsdf, want.tsdf) and _within_one_ulp(got.best, want.best)
    # the other cap: no weight reaches it
    loose = gpu_integrate(fresh(64), c2w, depth, colour, classes, mode)
    assert loose.info[0] == loose.weight.sum() and np.array_equal(loose.weight, T.integrate(fresh(64), c2w, T.FOCAL, depth, colour, classes, mode).weight)


@pytest.mark.parametrize("mode", [T.PLANAR, T.RAY])
def test_seven_views_in_one_call_equal_seven_calls(mode):
    for layout in ("wide", "packed"):
        c2w, depth, colour, classes = captures(mode, layout)
        a = gpu_integrate(fresh(3), c2w, depth, colour, classes, mode)
        b = gpu_integrate(fresh(3), c2w, depth, colour, classes, mode, one_by_one=True)
        for k in ("tsdf", "weight", "word", "best", "info"):
            assert getattr(a, k).tobytes() == getattr(b, k).tobytes(), (layout, k)


def test_a_view_that_misses_changes_nothing():
    c2w, depth, colour, classes = captures(T.PLANAR, "wide")
    before = gpu_integrate(fresh(), c2w[:4], depth[:4], colour[:4], classes[:4], T.PLANAR)
    after = gpu_integrate(before, c2w[4:5], depth[4:5], colour[4:5], classes[4:5], T.PLANAR)
    for k in ("tsdf", "weight", "word", "best", "info"):
        assert getattr(after, k).tobytes() == getattr(before, k).tobytes(), k
    none = gpu_integrate(before, c2w[:0], depth[:0], colour[:0], classes[:0], T.PLANAR)                  # n_views == 0
    assert none.tsdf.tobytes() == before.tsdf.tobytes() and none.info.tolist() == before.info.tolist()


# ------------------------------------------------------------------ general poses, skewed poses, the near plane, view lists beyond one wave
STATE = ("tsdf", "weight", "word", "best", "info")


def _assert_equals_restatement(got, want, mode, what):
    """The file's rule: planar mode to the byte; ray mode tsdf and best within one float32 ulp, the rest to the byte."""
    np.testing.assert_array_equal(got.weight, want.weight, err_msg=what)
    np.testing.assert_array_equal(got.word, want.word, err_msg=what)
    np.testing.assert_array_equal(got.info, want.info, err_msg=what)
    if mode == T.PLANAR:
        assert _same_bits(got.tsdf, want.tsdf) and _same_bits(got.best, want.best), what
    else:
        print(f"ray mode, {what}: tsdf bytes equal {_same_bits(got.tsdf, want.tsdf)}, best bytes equal {_same_bits(got.best, want.best)}")
        assert _within_one_ulp(got.tsdf, want.tsdf) and _within_one_ulp(got.best, want.best), what


def _assert_same_state(a, b, what):
    for k in STATE:
        assert getattr(a, k).tobytes() == getattr(b, k).tobytes(), (what, k)


def general(mode, layout):
    """`tsdf_ref.general_captures` in storage layout "wide" (RGBA / f32 / i64 with a patch of class 300) or "packed" (RGB / f16 / u8)."""
    c2w, depth, rgba, sem = T.general_captures(mode)
    if layout == "wide":
        sem = sem.astype(np.int64)
        sem[3, 4:12, 6:18] = 300
        return c2w, depth, rgba, sem
    return c2w, depth.astype(np.float16), np.ascontiguousarray(rgba[..., :3]), sem


def worded(max_weight=3, **kw):
    """A fresh volume whose words are not 0: the header leaves the initial word to the caller, and a point nothing reaches keeps it."""
    vol = T.volume(max_weight, **kw)
    vol.word = (np.arange(vol.word.size, dtype=np.uint32) * np.uint32(2654435761) | np.uint32(1)).reshape(vol.shape)
    return vol


@pytest.mark.parametrize("layout", ["wide", "packed"])
@pytest.mark.parametrize("mode", [T.PLANAR, T.RAY])
def test_general_poses_equal_the_restatement(mode, layout):
    """24 poses none of whose rotation entries is below 0.05 in magnitude: every index of the point chain and of the cull matters."""
    c2w, depth, colour, classes = general(mode, layout)
    want = T.integrate(worded(), c2w, T.FOCAL, depth, colour, classes, mode)
    got = gpu_integrate(worded(), c2w, depth, colour, classes, mode)
    assert want.info[0] > 3000 and want.info[3] > 0 and (want.weight == 3).any() and want.info[0] > want.weight.sum() and (want.info[4] > 0) == (layout == "wide")
    _assert_equals_restatement(got, want, mode, f"general poses, {layout}")


@pytest.mark.parametrize("mode", [T.PLANAR, T.RAY])
def test_skewed_poses_equal_the_restatement(mode):
    """The same captures under poses whose columns have norms 0.6, 1.04 and 1.9 and a shear: a cull that left the norms out of its bound
    drops points the header admits (tests/test_tsdf_cpu.py counts them).  The images mean nothing under such a pose; the bytes are held."""
    c2w, depth, colour, classes = general(mode, "wide")
    c2w = T.skewed(c2w)
    want = T.integrate(worded(), c2w, T.FOCAL, depth, colour, classes, mode)
    got = gpu_integrate(worded(), c2w, depth, colour, classes, mode)
    assert want.info[0] > 1000
    _assert_equals_restatement(got, want, mode, "skewed poses")


def test_min_depth_equals_the_restatement():
    """min_depth = 0.4 (step 3, and the cull's near plane) and max_depth = 0.6, below some stored depths (step 5)."""
    for mode in (T.PLANAR, T.RAY):
        c2w, depth, colour, classes = general(mode, "packed")
        assert (depth.astype(np.float32) > 0.6).any()
        want = T.integrate(worded(min_depth=0.4, max_depth=0.6), c2w, T.FOCAL, depth, colour, classes, mode)
        loose = T.integrate(worded(), c2w, T.FOCAL, depth, colour, classes, mode)
        assert 0 < want.info[0] < loose.info[0] and want.info[2] > loose.info[2]
        got = gpu_integrate(worded(min_depth=0.4, max_depth=0.6), c2w, depth, colour, classes, mode)
        _assert_equals_restatement(got, want, mode, "min_depth 0.4")


@pytest.mark.parametrize("mode", [T.PLANAR, T.RAY])
def test_six_hundred_views_equal_the_restatement(mode):
    """Two full chunks of 256 views and one of 88 (tests/test_tsdf_cpu.py says what they reach: blocks with more than 64 survivors from
    all four waves, a block first reached in the second chunk, a block never reached, tied views in different waves).  One call, 600
    calls and calls of 256 + 256 + 88 views give the same bytes, which are the restatement's."""
    c2w, depth, colour, classes = T.view_list(600, mode)
    want = T.integrate(worded(), c2w, T.FOCAL, depth, colour, classes, mode)
    one = gpu_integrate(worded(), c2w, depth, colour, classes, mode)
    if mode == T.PLANAR:
        _assert_equals_restatement(one, want, mode, "600 views in one call")
    else:                                                                        # a square root one ulp off numpy's may compound over 600 views: the three device runs are held to each other
        print("ray mode, 600 views: bytes equal the restatement's: " + ", ".join(f"{k} {_same_bits(getattr(one, k), getattr(want, k))}" for k in STATE))
    _assert_same_state(gpu_integrate(worded(), c2w, depth, colour, classes, mode, one_by_one=True), one, "600 calls")
    _assert_same_state(gpu_integrate(worded(), c2w, depth, colour, classes, mode, calls=[256, 256, 88]), one, "256 + 256 + 88")
    index, _ = T.block_table(one)
    never, start = index == T.B_NEVER, worded()
    assert never.sum() == 4 * 4 * 6 and (one.weight[index == T.B_LATE] > 0).any()
    for k in STATE[:4]:
        assert getattr(one, k)[never].tobytes() == getattr(start, k)[never].tobytes(), f"{k} of a block no view reaches"


def test_degenerate_poses_change_nothing_and_stop_nothing():
    """A pose holding a NaN, a camera infinitely far away and a camera exactly on a lattice point (q = 0 there: zd is 0 and xc / zd a NaN),
    in the middle of the general set.  The header defines all three: a NaN fails steps 3-4."""
    c2w, depth, colour, classes = general(T.PLANAR, "wide")
    nan_pose, far_pose, on_point = c2w[5].copy(), c2w[6].copy(), c2w[7].copy()
    nan_pose[1, 1] = np.nan
    far_pose[0, 3] = np.inf
    on_point[:, 3] = T.volume().points()[9, 4, 12]
    at = [0, 1, 2]
    put = lambda a, extra: np.concatenate([a[:12], extra, a[12:]])
    m = put(c2w, np.stack([nan_pose, far_pose, on_point]))
    d, c, k = (put(a, a[at]) for a in (depth, colour, classes))
    want = T.integrate(worded(), m, T.FOCAL, d, c, k, T.PLANAR)
    assert not T.project(T.volume(), on_point, T.W, T.H, T.FOCAL)[0][9, 4, 12] and T.project(T.volume(), on_point, T.W, T.H, T.FOCAL)[0].any()
    got = gpu_integrate(worded(), m, d, c, k, T.PLANAR)
    _assert_equals_restatement(got, want, T.PLANAR, "degenerate poses")
    keep = np.r_[0:12, 14:27]
    without = gpu_integrate(worded(), m[keep], d[keep], c[keep], k[keep], T.PLANAR)
    _assert_same_state(got, without, "the NaN and the infinite pose removed")
    alone = gpu_integrate(worded(), m[12:14], d[12:14], c[12:14], k[12:14], T.PLANAR)
    _assert_same_state(alone, worded(), "the NaN and the infinite pose alone")


# ------------------------------------------------------------------ lattice, mesh, attributes
def gpu_lattice(vol, min_weight):
    L, lib = _lib()
    n = int(np.prod(vol.shape))
    d_t, d_w, d_b = _dev(vol.tsdf), _dev(vol.weight), _dev(vol.best)
    outs = []
    for _ in range(2):
        vw, values = _guarded(n, torch.float32)
        cw, counts = _guarded(3, torch.int64)
        L.launch(lib.mnf_tsdf_lattice, L.ptr(d_t), L.ptr(d_w), L.ptr(d_b), *vol.cells, min_weight, L.ptr(values), L.ptr(counts), device=torch.device(DEV))
        torch.cuda.synchronize()
        _assert_guards(vw, n, "values")
        _assert_guards(cw, 3, "counts")
        outs.append((values.cpu().numpy().reshape(vol.shape), counts.cpu().numpy()))
    assert outs[0][0].tobytes() == outs[1][0].tobytes() and outs[0][1].tolist() == outs[1][1].tolist()
    return outs[0]


def gpu_extract(values, iso, origin, step, max_v, max_t, observed=True):
    L, lib = _lib()
    cells = tuple(n - 1 for n in values.shape)
    nbytes = int(lib.mnf_surface_extract_workspace_bytes(*cells))
    f3 = lambda v: (ctypes.c_float * 3)(*[float(np.float32(x)) for x in v])
    d_v = _dev(values)
    outs = []
    for _ in range(2):
        pw, pos = _guarded(3 * max_v, torch.int32)
        nw, nrm = _guarded(3 * max_v, torch.int32)
        tw, tri = _guarded(3 * max_t, torch.int32)
        iw, info = _guarded(4, torch.int64)
        ww, ws = _guarded(nbytes // 8, torch.int64)
        L.launch(lib.mnf_surface_extract_observed if observed else lib.mnf_surface_extract, L.ptr(d_v), *cells, float(iso), f3(origin), f3(step), max_v, max_t,
                 L.ptr(pos) if max_v else None, L.ptr(nrm) if max_v else None, L.ptr(tri) if max_t else None, L.ptr(info), L.ptr(ws), nbytes,
                 device=torch.device(DEV))
        torch.cuda.synchronize()
        for whole, k, what in ((pw, 3 * max_v, "positions"), (nw, 3 * max_v, "normals"), (tw, 3 * max_t, "triangles"), (iw, 4, "info"), (ww, nbytes // 8, "workspace")):
            _assert_guards(whole, k, what)
        outs.append([x.cpu().numpy() for x in (pos, nrm, tri, info)])
    assert all(a.tobytes() == b.tobytes() for a, b in zip(*outs))
    pos, nrm, tri, info = outs[0]
    return pos.reshape(max_v, 3), nrm.reshape(max_v, 3), tri.reshape(max_t, 3), info


def gpu_attrs(vol, positions, palette):
    L, lib = _lib()
    n = positions.shape[0]
    d_w, d_b, d_p, d_pal = _dev(vol.word.view(np.int32)), _dev(vol.best), _dev(positions), _dev(palette)
    outs = []
    for _ in range(2):
        cw, col = _guarded(3 * n, torch.uint8)
        lw, lab = _guarded(n, torch.int32)
        sw, sem = _guarded(3 * n, torch.uint8)
        L.launch(lib.mnf_tsdf_vertex_attrs, L.ptr(d_w), L.ptr(d_b), *vol.cells, _c3(vol.lo), float(vol.voxel), L.ptr(d_p), n, L.ptr(d_pal), palette.shape[0],
                 L.ptr(col), L.ptr(lab), L.ptr(sem), device=torch.device(DEV))
        torch.cuda.synchronize()
        for whole, k, what in ((cw, 3 * n, "colour"), (lw, n, "label"), (sw, 3 * n, "sem_colour")):
            _assert_guards(whole, k, what)
        outs.append({"colour": col.cpu().numpy().reshape(n, 3), "label": lab.cpu().numpy(), "sem_colour": sem.cpu().numpy().reshape(n, 3)})
    assert all(outs[0][k].tobytes() == outs[1][k].tobytes() for k in outs[0])
    return outs[0]


def test_lattice_mesh_and_attributes_equal_the_restatement():
    c2w, depth, colour, classes = captures(T.PLANAR, "wide")
    vol = gpu_integrate(fresh(), c2w, depth, colour, classes, T.PLANAR)                                  # the device's state: what follows reads it
    origin, step = vol.lo.astype(np.float32), np.full(3, np.float32(S))
    for min_weight in (1, 2):
        want_v, want_c = T.lattice(vol, min_weight)
        got_v, got_c = gpu_lattice(vol, min_weight)
        assert got_v.view(np.int32).tobytes() == want_v.view(np.int32).tobytes() and got_c.tolist() == want_c.tolist()
    values, _ = T.lattice(vol, 1)
    assert np.isnan(values).any()
    want = T.extract_observed(values, 0.0, origin, step)
    nv, nt = len(want["positions"]), len(want["triangles"])
    assert nv > 1000 and nt > 1000
    count = gpu_extract(values, 0.0, origin, step, 0, 0)[3]
    assert count.tolist() == [nv, nt, nv, nt]
    pos, nrm, tri, info = gpu_extract(values, 0.0, origin, step, nv, nt)
    assert info.tolist() == [nv, nt, 0, 0]
    assert pos.tobytes() == want["positions"].view(np.int32).tobytes() and nrm.tobytes() == want["normals"].view(np.int32).tobytes()
    np.testing.assert_array_equal(tri, want["triangles"])
    plain = gpu_extract(values, 0.0, origin, step, 0, 0, observed=False)[3]
    assert plain[1] > nt, "the unchanged entry wraps the observed region in a shell"
    rng = np.random.default_rng(3)
    extra = (vol.lo + rng.uniform(-0.1, 1.1, size=(300, 3)) * np.asarray(CELLS) * S).astype(np.float32)
    positions = np.concatenate([want["positions"], extra, np.array([[np.nan, 0, 0], [np.inf, -np.inf, 0]], np.float32)])
    palette = rng.integers(0, 256, size=(40, 3)).astype(np.uint8)                                       # class 255 (the label of 300) lies beyond it
    want_a = T.vertex_attrs(vol, positions, palette)
    got_a = gpu_attrs(vol, positions, palette)
    for k in ("colour", "label", "sem_colour"):
        np.testing.assert_array_equal(got_a[k], want_a[k], err_msg=k)
    assert (want_a["label"] == -1).any() and (want_a["label"] == 255).any() and (want_a["label"] >= 0).sum() > 1000


def test_observed_entry_equals_the_plain_one_without_nan():
    values = SF.ball((17, 13, 11), 3.9)
    frame = ((0.5, -1.25, 2.0), (0.25, 0.5, 0.125))
    n = gpu_extract(values, 0.0, *frame, 0, 0, observed=False)[3]
    a = gpu_extract(values, 0.0, *frame, int(n[0]), int(n[1]), observed=False)
    b = gpu_extract(values, 0.0, *frame, int(n[0]), int(n[1]), observed=True)
    assert n[0] > 100 and all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    short = gpu_extract(values, 0.0, *frame, int(n[0]) - 3, int(n[1]) - 5, observed=True)
    assert short[3].tolist() == [int(n[0]), int(n[1]), 3, 5]


# ------------------------------------------------------------------ argument errors
def test_argument_errors_are_refused_before_any_launch():
    L, lib = _lib()
    dev = torch.device(DEV)
    n = 21 * 10 * 22
    c2w, depth, colour, classes = captures(T.PLANAR, "wide")
    d_m, d_d, d_c, d_k = _dev(c2w), _dev(depth), _dev(colour), _dev(classes)
    tw, t = _guarded(n, torch.float32)
    ww, w = _guarded(n, torch.int32)
    dw, wd = _guarded(n, torch.int32)
    bw, b = _guarded(n, torch.float32)
    iw, info = _guarded(5, torch.int64)
    vw, values = _guarded(n, torch.float32)
    cw, counts = _guarded(3, torch.int64)
    aw, col = _guarded(12, torch.uint8)
    lw, lab = _guarded(4, torch.int32)
    pos = _dev(np.zeros((4, 3), np.float32))
    pal = _dev(np.zeros((4, 3), np.uint8))

    def off(tensor, nbytes):
        p = L.DevPtr(tensor.data_ptr() + nbytes)
        p.device = tensor.device
        return p

    nan, inf = float("nan"), float("inf")
    good = dict(t=L.ptr(t), w=L.ptr(w), wd=L.ptr(wd), b=L.ptr(b), X=20, Y=9, Z=21, lo=_c3(T.ROOM_LO), voxel=S, trunc=TRUNC, mw=64, dmin=0.0, dmax=10.0, m=L.ptr(d_m),
                V=7, W=T.W, H=T.H, focal=T.FOCAL, d=L.ptr(d_d), dt=0, c=L.ptr(d_c), cs=4, k=L.ptr(d_k), kt=1, mode=0, info=L.ptr(info))
    bad_integrate = [dict(t=None), dict(w=None), dict(wd=None), dict(b=None), dict(info=None), dict(m=None), dict(d=None), dict(c=None), dict(k=None), dict(lo=None),
                     dict(X=0), dict(Y=1025), dict(Z=-1), dict(lo=_c3([nan, 0, 0])), dict(voxel=0.0), dict(voxel=nan), dict(voxel=inf), dict(trunc=0.0),
                     dict(trunc=-1.0), dict(trunc=nan), dict(trunc=inf), dict(focal=0.0), dict(focal=nan), dict(focal=inf), dict(mw=0), dict(mw=-5),
                     dict(V=65536), dict(V=-1), dict(cs=2), dict(cs=5), dict(dt=2), dict(kt=2), dict(mode=2), dict(W=0), dict(H=16385), dict(dmin=-1.0),
                     dict(dmax=0.0), dict(dmax=inf), dict(t=off(t, 2)), dict(info=off(info, 4)), dict(m=off(d_m, 4)), dict(d=off(d_d, 2)), dict(k=off(d_k, 4))]
    for bad in bad_integrate:
        a = dict(good, **bad)
        with pytest.raises(L.MnfError):
            L.launch(lib.mnf_tsdf_integrate, a["t"], a["w"], a["wd"], a["b"], a["X"], a["Y"], a["Z"], a["lo"], a["voxel"], a["trunc"], a["mw"], a["dmin"], a["dmax"],
                     a["m"], a["V"], a["W"], a["H"], a["focal"], a["d"], a["dt"], a["c"], a["cs"], a["k"], a["kt"], a["mode"], a["info"], device=dev)
    good_l = dict(t=L.ptr(t), w=L.ptr(w), b=L.ptr(b), X=20, Y=9, Z=21, mw=1, v=L.ptr(values), c=L.ptr(counts))
    for bad in [dict(t=None), dict(w=None), dict(b=None), dict(v=None), dict(c=None), dict(X=0), dict(Z=1025), dict(mw=0), dict(c=off(counts, 4)), dict(v=off(values, 2))]:
        a = dict(good_l, **bad)
        with pytest.raises(L.MnfError):
            L.launch(lib.mnf_tsdf_lattice, a["t"], a["w"], a["b"], a["X"], a["Y"], a["Z"], a["mw"], a["v"], a["c"], device=dev)
    good_a = dict(wd=L.ptr(wd), b=L.ptr(b), X=20, Y=9, Z=21, lo=_c3(T.ROOM_LO), voxel=S, p=L.ptr(pos), n=4, pal=L.ptr(pal), np=4, col=L.ptr(col), lab=L.ptr(lab),
                  sem=None)
    for bad in [dict(wd=None), dict(b=None), dict(p=None), dict(lo=None), dict(X=0), dict(voxel=0.0), dict(voxel=nan), dict(n=-1), dict(n=1 << 31),
                dict(sem=L.ptr(col), pal=None), dict(sem=L.ptr(col), np=0), dict(np=-1), dict(p=off(pos, 2)), dict(lab=off(lab, 2))]:
        a = dict(good_a, **bad)
        with pytest.raises(L.MnfError):
            L.launch(lib.mnf_tsdf_vertex_attrs, a["wd"], a["b"], a["X"], a["Y"], a["Z"], a["lo"], a["voxel"], a["p"], a["n"], a["pal"], a["np"], a["col"], a["lab"],
                     a["sem"], device=dev)
    f3 = (ctypes.c_float * 3)(1.0, 1.0, 1.0)
    ws = torch.empty(int(lib.mnf_surface_extract_workspace_bytes(20, 9, 21)), dtype=torch.uint8, device=DEV)
    for bad in [dict(v=None), dict(X=0), dict(iso=nan), dict(o=None), dict(s=None), dict(mv=-1), dict(info=None), dict(ws=None), dict(nb=8)]:
        a = dict(dict(v=L.ptr(values), X=20, iso=0.0, o=f3, s=f3, mv=0, info=L.ptr(counts), ws=L.ptr(ws), nb=int(ws.numel())), **bad)
        with pytest.raises(L.MnfError):
            L.launch(lib.mnf_surface_extract_observed, a["v"], a["X"], 9, 21, a["iso"], a["o"], a["s"], a["mv"], 0, None, None, None, a["info"], a["ws"], a["nb"],
                     device=dev)
    torch.cuda.synchronize()
    for whole, k, what in ((tw, n, "tsdf"), (ww, n, "weight"), (dw, n, "word"), (bw, n, "best"), (iw, 5, "info"), (vw, n, "values"), (cw, 3, "counts"),
                           (aw, 12, "colour"), (lw, 4, "label")):
        _assert_guards(whole, k, what)
        assert (whole.cpu().numpy() == MARKS[whole.dtype]).all(), f"{what} was written by a refused call"


# ------------------------------------------------------------------ the Python surface
def _scene():
    from apnrf_amd import sensor as SN
    return SN.VoxelScene(T.room().copy(), T.ROOM_LO, S, device=DEV)


def _poses7(c2w):
    """xyz + quaternion (x, y, z, w) of the yaw-only poses."""
    out = []
    for m in c2w:
        yaw = np.arctan2(m[0, 2], m[0, 0])
        out.append([m[0, 3], m[1, 3], m[2, 3], 0.0, np.sin(yaw / 2), 0.0, np.cos(yaw / 2)])
    return np.asarray(out)


def test_volume_end_to_end(tmp_path):
    """`VoxelSim` -> `TsdfVolume.integrate` -> `extract_mesh` -> `SurfaceMesh.quality`, the sensor's RGBA and uint8 classes unsliced.  The
    state equals the restatement's on the captures the device made; the mesh carries the restatement's colours and labels.  The quality's
    bound: every vertex, hence every point of a triangle, lies within trunc + sqrt(3) voxel + |q| sqrt(2) / (2 focal) of matter
    (tests/test_tsdf_cpu.py derives it; |q| <= 0.8 m in this room), and the ground-truth cloud samples every occupied voxel's box at a
    quarter voxel, so a point of matter has a cloud point within sqrt(3) / 8 voxel."""
    from apnrf_amd import render as RD
    from apnrf_amd import sensor as SN
    from apnrf_amd.dataset import Dataset
    from apnrf_amd.tsdf import TsdfVolume
    scene = _scene()
    sim = SN.VoxelSim(scene, T.W, T.H, focal=T.FOCAL, far=100.0)
    c2w = T.room_poses(2)
    c2w_d = np.stack([RD.pose_to_c2w(p) for p in _poses7(c2w)])[:, :3, :]
    rgba, depth, sem = sim.sample_images_from_poses(_poses7(c2w), depth="ray")
    aabb = np.concatenate([T.ROOM_LO, T.ROOM_LO + np.asarray(CELLS) * S])
    vol = TsdfVolume(aabb, S, max_weight=3, device=DEV)
    assert vol.cells == CELLS and vol.trunc == 4 * S
    vol.integrate(depth, rgba, sem, torch.from_numpy(c2w_d).to(DEV), T.FOCAL, depth_along="ray")
    want = T.integrate(fresh(3), c2w_d, T.FOCAL, depth.cpu().numpy(), rgba.cpu().numpy(), sem.cpu().numpy(), T.RAY)
    assert list(vol.info().values()) == want.info.tolist()
    np.testing.assert_array_equal(vol.weight.cpu().numpy(), want.weight)
    np.testing.assert_array_equal(vol.word.cpu().numpy().view(np.uint32), want.word)
    assert _within_one_ulp(vol.tsdf.cpu().numpy(), want.tsdf)
    counts = vol.counts()
    assert counts["observed"] == int((want.weight > 0).sum()) and counts["points"] == 21 * 10 * 22 and 0.5 < counts["observed_fraction"] < 1
    palette = np.random.default_rng(8).integers(0, 256, size=(29, 3)).astype(np.uint8)
    mesh = vol.extract_mesh(palette=palette)
    state = fresh(3)
    state.tsdf, state.weight, state.best = vol.tsdf.cpu().numpy(), vol.weight.cpu().numpy(), vol.best.cpu().numpy()
    state.word = vol.word.cpu().numpy().view(np.uint32)
    ref = T.extract_observed(T.lattice(state)[0], 0.0, T.ROOM_LO.astype(np.float32), np.full(3, np.float32(S)))
    assert mesh.positions.cpu().numpy().tobytes() == ref["positions"].tobytes() and np.array_equal(mesh.triangles.cpu().numpy(), ref["triangles"])
    attrs = T.vertex_attrs(state, ref["positions"], palette)
    for k, got in (("colour", mesh.colour), ("label", mesh.label), ("sem_colour", mesh.sem_colour)):
        np.testing.assert_array_equal(got.cpu().numpy(), attrs[k], err_msg=k)
    # the quality against the room's own surfaces
    idx = np.argwhere(SR.occupied(T.room())).astype(np.float64)
    q = np.linspace(0.0, 1.0, 5)
    g = np.stack(np.meshgrid(q, q, q, indexing="ij"), axis=-1).reshape(-1, 3)
    g = g[((g == 0) | (g == 1)).any(axis=1)]                                                             # the box's faces
    gt = torch.from_numpy((T.ROOM_LO + (idx[:, None, :] + g[None]) * S).reshape(-1, 3).astype(np.float32)).to(DEV)
    quality = mesh.quality(gt, threshold=0.05, r_max=0.6)
    bound = TRUNC + np.sqrt(3.0) * S + 0.8 * np.sqrt(2.0) / (2 * T.FOCAL) + np.sqrt(3.0) / 8 * S
    print(f"tsdf mesh: {mesh.n_vertices} vertices, {mesh.n_triangles} triangles, accuracy {quality['accuracy']:.4f} m (bound {bound:.3f}), completion "
          f"{quality['completion']:.4f} m, precision {quality['precision']:.3f}")
    assert quality["truncated_pred"] == 0 and quality["accuracy"] <= bound
    # integrate_dataset: the same bytes, either storage layout, no image copied
    for packed in (False, True):
        ds = Dataset(training=False, save_fp=str(tmp_path / f"d{int(packed)}"), device=DEV, packed=packed)
        ds.update_data(rgba[..., :3], depth, sem, torch.from_numpy(c2w_d).to(DEV))
        a = TsdfVolume(aabb, S, max_weight=3, device=DEV)
        a.integrate_dataset(ds, [0, 1, 2, 4, 3, 5, 6], depth_along="ray")
        b = TsdfVolume(aabb, S, max_weight=3, device=DEV)
        order = torch.tensor([0, 1, 2, 4, 3, 5, 6], device=DEV)
        b.integrate(ds.depths[order], ds.images[order], ds.semantics[order], ds.camtoworlds[order], float(ds.K[0, 0]), depth_along="ray")
        for k in ("tsdf", "weight", "word", "best", "info_device"):
            assert torch.equal(getattr(a, k), getattr(b, k)), (packed, k)
        assert a.info()["applied"] > 3000
    vol.clear()
    assert vol.info()["applied"] == 0 and vol.counts()["observed"] == 0 and vol.extract_mesh().n_triangles == 0
    with pytest.raises(L_error()):
        TsdfVolume(aabb, S, device="cpu")


def test_volume_takes_six_hundred_float32_poses(tmp_path):
    """`TsdfVolume.integrate` with the 600 views' poses as a float32 [V,4,4] device tensor is the C ABI on the float32-rounded poses, and
    `integrate_dataset` with an id list of three runs (one longer than a chunk, out of order) is `integrate` on the gathered views."""
    from apnrf_amd.dataset import Dataset
    from apnrf_amd.tsdf import TsdfVolume
    c2w, depth, rgba, sem = T.view_list(600, T.PLANAR)
    c2w32 = c2w.astype(np.float32)
    m44 = np.concatenate([c2w32, np.broadcast_to(np.array([0, 0, 0, 1], np.float32), (600, 1, 4))], axis=1)
    aabb = np.concatenate([T.ROOM_LO, T.ROOM_LO + np.asarray(CELLS) * S])
    vol = TsdfVolume(aabb, S, max_weight=3, device=DEV)
    vol.integrate(_dev(depth), _dev(rgba), _dev(sem), _dev(m44), T.FOCAL, depth_along="z")
    want = gpu_integrate(fresh(3), c2w32.astype(np.float64), depth, rgba, sem, T.PLANAR)
    assert want.info[0] > 100000 and (c2w32.astype(np.float64) != c2w).any()
    assert list(vol.info().values()) == want.info.tolist()
    for k in ("tsdf", "weight", "best"):
        assert getattr(vol, k).cpu().numpy().tobytes() == getattr(want, k).tobytes(), k
    assert vol.word.cpu().numpy().view(np.uint32).tobytes() == want.word.tobytes()
    ids = list(range(280, 600)) + list(range(0, 260)) + list(range(270, 280))
    order = torch.tensor(ids, device=DEV)
    for packed in (False, True):
        ds = Dataset(training=False, save_fp=str(tmp_path / f"d{int(packed)}"), device=DEV, packed=packed)
        ds.update_data(_dev(np.ascontiguousarray(rgba[..., :3])), _dev(depth), _dev(sem), _dev(c2w32))
        assert float(ds.K[0, 0]) == T.FOCAL
        a = TsdfVolume(aabb, S, max_weight=3, device=DEV)
        a.integrate_dataset(ds, ids)
        b = TsdfVolume(aabb, S, max_weight=3, device=DEV)
        b.integrate(ds.depths[order], ds.images[order], ds.semantics[order], ds.camtoworlds[order], T.FOCAL)
        for k in ("tsdf", "weight", "word", "best", "info_device"):
            assert torch.equal(getattr(a, k), getattr(b, k)), (packed, k)
        assert a.info()["applied"] > 100000 and not torch.equal(a.tsdf, vol.tsdf), "the order of the runs is the order of fusion"


def L_error():
    from apnrf_amd import _lib as L
    return L.MnfError
