"""GPU tests of the mesh-quality unit (csrc/cloud.hip, apnrf_amd/cloud.py) against the numpy restatement tests/cloud_ref.py, which
tests/test_cloud_cpu.py holds to the definition.  Sampled points and `face` are compared bit for bit, nearest indices by `array_equal` and
distances by their bits against brute force over all pairs, counts and confusion exactly; only the sums have a tolerance, the bound of any
summation order.  Outputs and workspaces of the C ABI are allocated with guard elements on both sides."""
import ctypes

import numpy as np
import pytest
import torch

import cloud_ref as CR
import surface_ref as SR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64
MARK32, MARK64 = -0x5A5A5A5B, -0x5A5A5A5A5A5A5A5B


def _dev(a):
    return torch.from_numpy(np.array(a, copy=True, order="C")).to(DEV)


def _guarded(n, dtype, mark):
    whole = torch.full((n + 2 * GUARD,), mark, dtype=dtype, device=DEV)
    return whole, whole[GUARD:GUARD + n]


def _assert_guards(whole, n, mark, what):
    host = whole.cpu().numpy()
    assert (host[:GUARD] == mark).all() and (host[GUARD + n:] == mark).all(), f"{what}: written outside its bounds"


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


# ------------------------------------------------------------------ sampling: the meshes and their reference clouds, computed once
def _mesh_one():
    return np.array([[0.1, 0.2, 0.3], [0.473, 0.251, 0.334], [0.157, 0.433, 0.262]], np.float32), np.array([[0, 1, 2]], np.int32), 0.01


def _mesh_many():
    rng = np.random.default_rng(11)
    base = rng.random((300, 1, 3)) * 2.0 - 1.0
    pos = (base + (rng.random((300, 3, 3)) - 0.5) * 0.17).reshape(900, 3).astype(np.float32)
    tri = rng.permutation(900).astype(np.int32).reshape(300, 3)      # twenty triangles of unrelated vertices too: sides up to the cube's diagonal
    tri[:280] = np.arange(840, dtype=np.int32).reshape(280, 3)
    return pos, tri, 0.013


def _mesh_special():
    pos = np.array([[0, 0, 0], [0.31, 0.02, 0.05], [0.04, 0.27, 0.01], [np.nan, 0, 0], [0.3, np.inf, 0], [0.31, 0.02, 0.05]], np.float32)
    tri = np.array([[0, 1, 2], [0, 0, 2], [0, 1, 0], [1, 1, 1], [1, 5, 2], [0, 1, 3], [4, 1, 2], [0, 1, 6], [-1, 1, 2], [2, 1, 0]], np.int32)
    return pos, tri, 0.0173


def _mesh_exact():
    # 0.5 / 0.125 = 4 and every b / res of this triangle is computed without any rounding: the counts are exact integers by arithmetic
    return np.array([[0, 0, 0], [0.5, 0, 0], [0, 0.25, 0]], np.float32), np.array([[0, 1, 2]], np.int32), 0.125


def _mesh_inexact():
    return np.array([[0, 0, 0], [0.55, 0, 0], [0, 0.26, 0.01]], np.float32), np.array([[0, 1, 2]], np.int32), 0.125


def _mesh_sliver():
    return np.array([[0, 0, 0], [1.003, 0.002, 0], [0.0007, 0.0003, 0.0001], [1.0037, 0.0, 0.00004]], np.float32), np.array([[0, 1, 2], [0, 3, 2]], np.int32), 0.01


def _mesh_big():
    pos = np.array([[0, 0, 0], [0.013, 0.001, 0], [0, 0.017, 0.002], [0.5, 0.5, 0.5], [1.273, 0.51, 0.52], [0.49, 1.288, 0.47], [0.02, 0, 0.011]], np.float32)
    tri = np.array([[0, 1, 2], [2, 1, 6], [3, 4, 5], [0, 6, 1], [6, 2, 0]], np.int32)
    return pos, tri, 0.01


MESHES = {"one": _mesh_one, "many": _mesh_many, "special": _mesh_special, "exact": _mesh_exact, "inexact": _mesh_inexact, "sliver": _mesh_sliver,
          "big": _mesh_big}
_SAMPLED = {}


def sampled(name):
    if name not in _SAMPLED:
        pos, tri, res = MESHES[name]()
        pts, face = CR.sample_triangles(pos, tri, res)
        rows = CR.triangle_rows(pos, tri, res)
        for a in (pos, tri, pts, face):
            a.setflags(write=False)
        _SAMPLED[name] = (pos, tri, res, pts, face, rows)
    return _SAMPLED[name]


def gpu_sample(pos, tri, res, max_rows, max_points):
    """mnf_cloud_sample_triangles through the C ABI -> (points bits [max_points,3], face [max_points], info [2]) as the call left them."""
    from apnrf_amd import _lib as L
    lib = L.load_library()
    V, T = len(pos), len(tri)
    nbytes = int(lib.mnf_cloud_sample_triangles_workspace_bytes(T, max_rows))
    assert nbytes > 0 and nbytes % 8 == 0
    pw, pts = _guarded(3 * max_points, torch.int32, MARK32)
    fw, face = _guarded(max_points, torch.int32, MARK32)
    iw, info = _guarded(2, torch.int64, MARK64)
    ww, ws = _guarded(nbytes // 8, torch.int64, MARK64)
    d_pos, d_tri = _dev(pos), _dev(tri)
    L.launch(lib.mnf_cloud_sample_triangles, L.ptr(d_pos), V, L.ptr(d_tri), T, float(res), max_rows, max_points, L.ptr(pts) if max_points else None,
             L.ptr(face) if max_points else None, L.ptr(info), L.ptr(ws), nbytes, device=torch.device(DEV))
    torch.cuda.synchronize()
    for whole, n, mark, what in ((pw, 3 * max_points, MARK32, "points"), (fw, max_points, MARK32, "face"), (iw, 2, MARK64, "info"),
                                 (ww, nbytes // 8, MARK64, "workspace")):
        _assert_guards(whole, n, mark, what)
    return pts.cpu().numpy().reshape(max_points, 3), face.cpu().numpy(), info.cpu().numpy()


@pytest.mark.parametrize("name", list(MESHES))
def test_sampling_matches_the_restatement(name):
    pos, tri, res, want, want_face, rows = sampled(name)
    P = len(want)
    if name != "exact":                                             # no count may hinge on the last bit of a square root or a division
        ratios = CR.triangle_ratios(pos, tri, res)
        assert len(ratios) and np.abs(ratios - np.round(ratios)).min() > 1e-9
    pts, face, info = gpu_sample(pos, tri, res, rows, P)
    assert info.tolist() == [P, 0]
    np.testing.assert_array_equal(pts, _bits(want))
    np.testing.assert_array_equal(face, want_face)
    # a counting call; a capacity below the count; roomy capacities: the counts stay and the rest of the buffers is left alone
    assert gpu_sample(pos, tri, res, rows, 0)[2].tolist() == [P, P]
    short = P - min(P, 7)
    pts1, face1, info1 = gpu_sample(pos, tri, res, rows + 3, short)
    assert info1.tolist() == [P, P - short]
    np.testing.assert_array_equal(pts1, _bits(want)[:short])
    np.testing.assert_array_equal(face1, want_face[:short])
    pts2, face2, info2 = gpu_sample(pos, tri, res, rows + 300, P + 5)
    assert info2.tolist() == [P, 0] and (pts2[P:] == MARK32).all() and (face2[P:] == MARK32).all()
    np.testing.assert_array_equal(pts2[:P], _bits(want))
    np.testing.assert_array_equal(face2[:P], want_face)
    # fewer rows than the mesh has: the rows are reported and nothing is written
    for max_rows in (0, rows - 1):
        pts3, face3, info3 = gpu_sample(pos, tri, res, max_rows, P)
        assert info3.tolist() == [-1, rows] and (pts3 == MARK32).all() and (face3 == MARK32).all()


def test_sampling_shapes_are_what_they_are_meant_to_be():
    assert len(sampled("one")[1]) == 1 and len(sampled("many")[1]) == 300 and sampled("many")[5] > 256 and len(sampled("many")[3]) > 4 * 256
    big = sampled("big")
    per_face = np.bincount(big[4], minlength=5)
    assert 2800 < per_face[2] < 3400 and per_face[[0, 1, 3, 4]].max() < 20
    special = sampled("special")
    assert np.bincount(special[4], minlength=10).tolist()[1:9] == [3, 3, 3, 3, 3, 3, 0, 0]
    sliver = sampled("sliver")
    assert sliver[5] == 2 + 101 + 101 and len(sliver[3]) == 2 * (3 + 101)      # one point per row


def test_sample_mesh_points_python():
    from apnrf_amd.cloud import sample_mesh_points
    from apnrf_amd.surface import SurfaceMesh
    for name in ("many", "sliver", "big"):
        pos, tri, res, want, want_face, _ = sampled(name)
        pts, face = sample_mesh_points(_dev(pos), _dev(tri), res)
        assert pts.is_cuda and pts.dtype == torch.float32 and face.dtype == torch.int32
        np.testing.assert_array_equal(_bits(pts.cpu().numpy()), _bits(want))
        np.testing.assert_array_equal(face.cpu().numpy(), want_face)
    # a resolution at which one triangle has thousands of rows of a few points each
    pos, tri, _ = _mesh_sliver()
    want, want_face = CR.sample_triangles(pos, tri[:1], 0.00019)
    assert CR.triangle_rows(pos, tri[:1], 0.00019) > 4096
    mesh = SurfaceMesh(_dev(pos), None, _dev(tri[:1]), None)
    pts, face = sample_mesh_points(mesh, resolution=0.00019)
    np.testing.assert_array_equal(_bits(pts.cpu().numpy()), _bits(want))
    np.testing.assert_array_equal(face.cpu().numpy(), want_face)
    empty = sample_mesh_points(_dev(pos), torch.zeros(0, 3, dtype=torch.int32, device=DEV), 0.01)
    assert tuple(empty[0].shape) == (0, 3) and tuple(empty[1].shape) == (0,)


# ------------------------------------------------------------------ nearest neighbour
ANISO = (0.0, 0.0, 0.0, 1.75, 0.75, 1.25)                           # 7 x 3 x 5 cells at r_max = 0.25


def _box(v):
    return (ctypes.c_float * 6)(*[float(x) for x in v])


def gpu_nearest(q, t, r_max, box):
    """mnf_cloud_nearest through the C ABI -> (dist bits [n], index [n]); the guards around outputs and workspace are checked."""
    from apnrf_amd import _lib as L
    lib = L.load_library()
    q, t = np.ascontiguousarray(q, np.float32).reshape(-1, 3), np.ascontiguousarray(t, np.float32).reshape(-1, 3)
    n, m = len(q), len(t)
    nbytes = int(lib.mnf_cloud_nearest_workspace_bytes(n, m, _box(box), float(r_max)))
    assert nbytes > 0 and nbytes % 16 == 0
    iw, index = _guarded(n, torch.int32, MARK32)
    dw, dist = _guarded(n, torch.int32, MARK32)
    ww, ws = _guarded(nbytes // 8, torch.int64, MARK64)             # 64 guard elements of 8 bytes keep the 16-byte alignment of torch's allocation
    d_q, d_t = _dev(q), _dev(t)
    L.launch(lib.mnf_cloud_nearest, L.ptr(d_q), n, L.ptr(d_t) if m else None, m, float(r_max), _box(box), L.ptr(index), L.ptr(dist), L.ptr(ws), nbytes,
             device=torch.device(DEV))
    torch.cuda.synchronize()
    for whole, k, mark, what in ((iw, n, MARK32, "index"), (dw, n, MARK32, "dist"), (ww, nbytes // 8, MARK64, "workspace")):
        _assert_guards(whole, k, mark, what)
    return dist.cpu().numpy(), index.cpu().numpy()


def _assert_nearest(q, t, r_max, box):
    want_d, want_i = CR.nearest(q, t, r_max)
    dist, index = gpu_nearest(q, t, r_max, box)
    np.testing.assert_array_equal(index, want_i)
    np.testing.assert_array_equal(dist, _bits(want_d))
    return want_i


_CLOUDS = {}


def random_clouds():
    if not _CLOUDS:
        rng = np.random.default_rng(3)
        scale = np.array(ANISO[3:], np.float32)
        _CLOUDS["q"] = (rng.random((4000, 3), dtype=np.float32) * scale).astype(np.float32)
        _CLOUDS["t"] = (rng.random((3000, 3), dtype=np.float32) * scale).astype(np.float32)
        _CLOUDS["q"].setflags(write=False)
        _CLOUDS["t"].setflags(write=False)
    return _CLOUDS["q"], _CLOUDS["t"]


@pytest.mark.parametrize("box", [ANISO, (0.5, 0.5, 0.5, 0.5, 0.5, 0.5), (0.3, 0.1, 0.2, 1.1, 0.4, 0.9)], ids=["7x3x5", "one_cell", "inner_box"])
def test_nearest_random_clouds(box):
    q, t = random_clouds()
    found = _assert_nearest(q, t, 0.0625 if box == ANISO else 0.25, box)      # 0.0625 in the 7 x 3 x 5 box: the list grows to 28 x 12 x 20 cells, many empty
    assert 0 < (found >= 0).sum()
    if box == ANISO:
        assert (found < 0).sum() > 100
        _assert_nearest(q, t, 0.25, box)


def test_nearest_single_points():
    q, t = random_clouds()
    _assert_nearest(q[:300], t[:1], 0.5, ANISO)
    _assert_nearest(q[:1], t, 0.25, ANISO)
    _assert_nearest(q[:1], t[:1], 2.5, ANISO)
    dist, index = gpu_nearest(q[:5], np.zeros((0, 3), np.float32), 0.25, ANISO)
    assert (index == -1).all() and (dist == _bits(np.float32(0.25))).all()


def test_nearest_one_crowded_cell():
    rng = np.random.default_rng(8)
    t = (0.3 + 0.2 * rng.random((5000, 3), dtype=np.float32)).astype(np.float32)      # one cell of the 7 x 3 x 5 list: five staging chunks
    q = (0.2 + 0.4 * rng.random((300, 3), dtype=np.float32)).astype(np.float32)
    _assert_nearest(q, t, 0.25, ANISO)


def test_nearest_duplicates_take_the_lowest_index():
    q, t = random_clouds()
    tt = np.concatenate([t[:700][::-1], t[:700], t[:700]])
    qq = np.concatenate([q[:500], t[:200]])                         # and queries that sit on a target: distance 0
    found = _assert_nearest(qq, tt, 0.25, ANISO)
    assert (found[500:] < 700).all() and (found[500:] >= 500).all()


def test_nearest_at_the_radius_and_just_beyond():
    beyond = np.nextafter(np.float32(0.25), np.float32(1))
    t = np.zeros((1, 3), np.float32)                                # at the origin: the four queries are +-0.25 and +-nextafter exactly, two outside the box
    for axis in range(3):
        q = np.repeat(t, 4, axis=0)
        q[0, axis] += np.float32(0.25)
        q[1, axis] -= np.float32(0.25)
        q[2, axis] += beyond
        q[3, axis] -= beyond
        dist, index = gpu_nearest(q, t, 0.25, ANISO)
        assert index.tolist() == [0, 0, -1, -1] and (dist == _bits(np.float32(0.25))).all()
        _assert_nearest(q, t, 0.25, ANISO)


def test_nearest_outside_the_box_and_non_finite():
    box = (0.0, 0.0, 0.0, 1.0, 1.0, 1.0)
    t = np.array([[0.99, 0.5, 0.5], [0.01, 0.5, 0.5], [1.4, 1.4, 1.4], [-3.0, 0.5, 0.5], [np.nan, 0.5, 0.5], [0.9, np.inf, 0.5], [0.9, 0.5, -np.inf],
                  [0.5, 0.5, 0.5]], np.float32)
    q = np.array([[1.2, 0.5, 0.5], [1.3, 0.5, 0.5], [-0.2, 0.5, 0.5], [-0.3, 0.5, 0.5], [1.5, 1.5, 1.5], [1.6, 1.6, 1.6], [-3.1, 0.4, 0.5], [1e30, 0.5, 0.5],
                  [-1e30, -1e30, 1e30], [np.nan, 0.5, 0.5], [0.5, np.inf, 0.5], [0.5, 0.5, -np.inf], [0.9, 0.6, 0.5], [0.5, 0.5, 0.5], [3e38, 3e38, 3e38]], np.float32)
    found = _assert_nearest(q, t, 0.25, box)
    assert found.tolist() == [0, -1, 1, -1, 2, -1, 3, -1, -1, -1, -1, -1, 0, 7, -1]


def test_nearest_empty_cells_all_round():
    t = np.array([[0.1, 0.1, 0.1], [3.9, 2.9, 1.9], [2.0, 1.5, 1.0], [2.01, 1.5, 1.0]], np.float32)
    rng = np.random.default_rng(2)
    q = np.concatenate([t + np.float32(0.03), t - np.float32(0.2), (rng.random((600, 3)) * np.array([4.0, 3.0, 2.0])).astype(np.float32)])
    found = _assert_nearest(q, t, 0.125, (0, 0, 0, 4, 3, 2))
    assert (found[:4] >= 0).all() and (found[4:8] == -1).all()


def test_nearest_python():
    from apnrf_amd.cloud import nearest
    q, t = random_clouds()
    want_d, want_i = CR.nearest(q, t, 0.25)
    for box in (None, ANISO, torch.tensor(ANISO)):
        dist, index = nearest(_dev(q), _dev(t), 0.25, box=box)
        assert dist.is_cuda and dist.dtype == torch.float32 and index.dtype == torch.int32
        np.testing.assert_array_equal(index.cpu().numpy(), want_i)
        np.testing.assert_array_equal(_bits(dist.cpu().numpy()), _bits(want_d))


# ------------------------------------------------------------------ reduction
def gpu_stats(dist, index, query, thr, r_max, m, ql=None, tl=None, C=0):
    from apnrf_amd import _lib as L
    lib = L.load_library()
    n = len(dist)
    cw, counts = _guarded(3, torch.int64, MARK64)
    sw, sums = _guarded(2, torch.float64, float(MARK32))
    fw, conf = _guarded(C * C, torch.int64, MARK64)
    d = [None if a is None else _dev(a) for a in (np.asarray(dist, np.float32), np.asarray(index, np.int32), query, ql, tl)]
    L.launch(lib.mnf_cloud_distance_stats, L.ptr(d[0]), L.ptr(d[1]), L.ptr(d[2]), n, float(thr), float(r_max), L.ptr(d[3]), L.ptr(d[4]), m, C, L.ptr(counts),
             L.ptr(sums), L.ptr(conf) if C else None, device=torch.device(DEV))
    torch.cuda.synchronize()
    _assert_guards(cw, 3, MARK64, "counts")
    _assert_guards(sw, 2, float(MARK32), "sums")
    _assert_guards(fw, C * C, MARK64, "confusion")
    return counts.cpu().numpy(), sums.cpu().numpy(), conf.cpu().numpy().reshape(C, C)


def test_distance_stats():
    q, t = random_clouds()
    q = q.copy()
    q[5, 1], q[77, 0], q[3999, 2] = np.nan, np.inf, -np.inf
    r_max = np.float32(0.0625)
    dist, index = CR.nearest(q, t, r_max)
    rng = np.random.default_rng(4)
    C = 5
    ql = rng.integers(-1, C + 1, len(q)).astype(np.int32)           # -1 and C are outside [0, C): ignored
    tl = rng.integers(-1, C + 1, len(t)).astype(np.int32)
    for thr in (0.0, float(r_max), 0.03):
        want_c, want_s, want_f = CR.distance_stats(dist, index, thr, len(t), q, ql, tl, C)
        counts, sums, conf = gpu_stats(dist, index, q, thr, r_max, len(t), ql, tl, C)
        assert counts.tolist() == want_c.tolist()
        np.testing.assert_array_equal(conf, want_f)
        for k, members in ((0, want_c[0]), (1, want_c[1])):
            assert abs(sums[k] - want_s[k]) <= int(members) * 2.0 ** -53 * want_s[k], (k, sums[k], want_s[k])
    assert want_c[0] == len(q) - 3 and 0 < want_c[1] < want_c[0] and want_f.sum() < want_c[2]
    # without the queries every entry counts; without labels no matrix is touched
    want_c, want_s, _ = CR.distance_stats(dist, index, 0.03, len(t))
    counts, sums, _ = gpu_stats(dist, index, None, 0.03, r_max, len(t))
    assert counts.tolist() == want_c.tolist() and want_c[0] == len(q)
    assert abs(sums[0] - want_s[0]) <= len(q) * 2.0 ** -53 * want_s[0]
    # an index outside [0, m) is not found
    counts, _, _ = gpu_stats(dist, index, q, 0.03, r_max, 100)
    assert counts.tolist() == CR.distance_stats(dist, index, 0.03, 100, q)[0].tolist()


# ------------------------------------------------------------------ mesh_quality
STEP = 1.0 / 32


def _ball_mesh(shape, radius):
    from apnrf_amd.surface import extract_lattice_surface
    return extract_lattice_surface(_dev(SR.ball(shape, radius)), 0.0, (0.0, 0.0, 0.0), (STEP, STEP, STEP))


def _centre(shape):
    return ((np.array(shape, np.float64) - 1.0) / 2.0 + 0.13) * STEP


def _sphere_points(n, radius, centre):
    """n points of a Fibonacci spiral on a sphere, float32."""
    k = np.arange(n, dtype=np.float64) + 0.5
    z = 1.0 - 2.0 * k / n
    phi = k * (np.pi * (3.0 - np.sqrt(5.0)))
    s = np.sqrt(1.0 - z * z)
    return (np.stack([s * np.cos(phi), s * np.sin(phi), z], axis=1) * radius + centre).astype(np.float32)


def test_a_mesh_against_its_own_sampling():
    from apnrf_amd.cloud import mesh_quality, sample_mesh_points
    mesh = _ball_mesh((13, 13, 13), 4.0)
    points, _ = sample_mesh_points(mesh, resolution=0.01)
    for got in (mesh_quality(mesh, points, resolution=0.01), mesh.quality(points, resolution=0.01), mesh_quality(points, points)):
        assert got["accuracy"] == 0.0 and got["completion"] == 0.0 and got["completion_ratio"] == 1.0
        assert got["precision"] == 1.0 and got["recall"] == 1.0 and got["fscore"] == 1.0 and got["chamfer"] == 0.0
        assert got["n_pred"] == got["n_gt"] == int(points.shape[0]) and got["truncated_pred"] == got["truncated_gt"] == 0
        assert "confusion" not in got
    far = mesh_quality(mesh, points + 1.0, resolution=0.01)         # nothing within r_max = 0.2: all truncated, and the result says so
    assert far["accuracy"] == far["completion"] == float(np.float32(0.2)) and far["fscore"] == 0.0
    assert far["truncated_pred"] == far["n_pred"] and far["truncated_gt"] == far["n_gt"]


def test_a_ball_against_a_larger_ball():
    """The mesh of a ball of radius 8 / 32 against 20 000 points on the sphere of radius 9 / 32: accuracy and completion are the offset 1 / 32.
    Tolerance: the mesh's own faceting error.  Measured on the CPU restatement (surface_ref.extract + cloud_ref.sample_triangles at 0.01), the
    sampled points of this mesh lie between 0.0014396 inside the sphere of radius 8 / 32 and on it: f = 0.00144.
    The restatement itself (cloud_ref.quality on the same two clouds, brute force, 36 s on a host) gives accuracy 0.031823707343304766 and
    completion 0.032021741963736715, recorded below; the device sums the same float32 distances in another order, so it is held to them within
    the bound of any summation order, (n + 2) 2^-53 relative (the two more: the sum's and the quotient's own rounding)."""
    from apnrf_amd.cloud import mesh_quality
    shape, off, f = (25, 25, 25), 1.0 / 32, 0.00144
    restated = {"accuracy": (0.031823707343304766, 53580), "completion": (0.032021741963736715, 20000)}
    mesh = _ball_mesh(shape, 8.0)
    gt = _dev(_sphere_points(20000, 9.0 * STEP, _centre(shape)))
    got = mesh_quality(mesh, gt, resolution=0.01, threshold=0.05)
    print("ball against ball:", {k: got[k] for k in ("accuracy", "completion", "completion_ratio", "precision", "fscore", "chamfer", "n_pred", "n_gt")})
    assert abs(got["accuracy"] - off) <= f and abs(got["completion"] - off) <= f
    for key, (want, n) in restated.items():
        assert abs(got[key] - want) <= (n + 2) * 2.0 ** -53 * want, (key, got[key], want)
    assert got["completion_ratio"] == 1.0 and got["precision"] == 1.0 and got["fscore"] == 1.0
    assert got["chamfer"] == 0.5 * (got["accuracy"] + got["completion"])
    assert got["n_gt"] == 20000 and got["n_pred"] == 53580 and got["truncated_pred"] == got["truncated_gt"] == 0
    tight = mesh_quality(mesh, gt, resolution=0.01, threshold=0.029)                  # below off - f = 0.0298: nothing is within
    assert tight["completion_ratio"] == 0.0 and tight["precision"] == 0.0 and tight["fscore"] == 0.0 and tight["truncated_gt"] == 0


def test_labels_split_by_hemisphere():
    from apnrf_amd.cloud import mesh_quality
    shape = (13, 13, 13)
    mesh = _ball_mesh(shape, 4.0)
    c = _centre(shape)
    pos, tri = mesh.positions.cpu().numpy(), mesh.triangles.cpu().numpy()
    vlabel = (pos[:, 0] > c[0]).astype(np.int32)
    gt = _sphere_points(4000, 5.0 * STEP, c)
    glabel = (gt[:, 0] > c[0]).astype(np.int32)
    got = mesh_quality(mesh, _dev(gt), gt_labels=_dev(glabel), pred_labels=_dev(vlabel), resolution=0.01, threshold=0.05, num_classes=3)
    # the same by the restatement: each sampled point takes the label of its triangle's first vertex
    pts, face = CR.sample_triangles(pos, tri, 0.01)
    plabel = vlabel[tri[face, 0]]
    d, i = CR.nearest(gt, pts, 0.2)
    _, _, want = CR.distance_stats(d, i, 0.05, len(pts), gt, glabel, plabel, 3)
    np.testing.assert_array_equal(got["confusion"], want)
    conf = got["confusion"]
    assert conf.sum() == 4000 and conf[2].sum() == 0 and conf[:, 2].sum() == 0
    # the two hemispheres agree except next to the plane between them, where a triangle reaches across it: a gt point is within 0.0344 of its
    # nearest sample (the largest distance d above is 0.03431) and the sample within a cell's diagonal of the vertex that labels it
    assert d.max() <= 0.0344
    band = 0.0344 + np.sqrt(3.0) * STEP
    assert conf[0, 1] + conf[1, 0] <= (np.abs(gt[:, 0] - c[0]) <= band).sum() and conf[0, 0] > 10 * conf[0, 1] and conf[1, 1] > 5 * conf[1, 0]
    assert got["label_accuracy"] == (conf[0, 0] + conf[1, 1]) / 4000.0
    iou = [conf[k, k] / (conf[k].sum() + conf[:, k].sum() - conf[k, k]) for k in (0, 1)]
    assert got["miou"] == pytest.approx(sum(iou) / 2.0, rel=1e-12)
    # labels from the mesh itself (SurfaceMesh.label), and the default class count
    mesh.label = _dev(vlabel)
    again = mesh.quality(_dev(gt), gt_labels=_dev(glabel), resolution=0.01)
    np.testing.assert_array_equal(again["confusion"], want[:2, :2])
