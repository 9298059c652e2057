"""The numpy restatement of the mesh-quality unit, tests/cloud_ref.py, held to known answers of include/mi355nerf.h ("mesh quality"), and the
part of the C ABI that needs no GPU: the workspace sizes, the argument errors (refused before any HIP call) and the PLY reader of
apnrf_amd.cloud.  tests/test_gpu_cloud.py holds the device to the restatement."""
import ctypes

import numpy as np
import pytest

import cloud_ref as CR


# ------------------------------------------------------------------ the restatement
def test_right_triangle_known_points():
    pos = np.array([[0, 0, 0], [0.5, 0, 0], [0, 0.25, 0]], np.float32)
    pts, face = CR.sample_triangles(pos, np.array([[0, 1, 2]], np.int32), 0.125)
    want = [[0, 0, 0], [0.5, 0, 0], [0, 0.25, 0],                   # the vertices
            [0, 0, 0], [0, 0.125, 0],                               # k = 0: b = 0.25 -> 2
            [0.125, 0, 0], [0.125, 0.125, 0],                       # k = 1: b = 0.1875 -> 2
            [0.25, 0, 0],                                           # k = 2: b = 0.125 -> 1
            [0.375, 0, 0]]                                          # k = 3: b = 0.0625 -> 1
    assert pts.dtype == np.float32 and face.dtype == np.int32
    np.testing.assert_array_equal(pts, np.array(want, np.float32))
    np.testing.assert_array_equal(face, np.zeros(9, np.int32))


def test_degenerate_triangles_give_their_vertices_and_bad_indices_nothing():
    pos = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [np.nan, 0, 0]], np.float32)
    tris = np.array([[0, 0, 2], [0, 1, 0], [1, 1, 1], [0, 1, 3], [0, 1, 4], [-1, 1, 2], [0, 1, 2]], np.int32)
    pts, face = CR.sample_triangles(pos, tris, 0.5)
    assert face.tolist() == [0] * 3 + [1] * 3 + [2] * 3 + [3] * 3 + [6] * (3 + 2 + 1)
    np.testing.assert_array_equal(pts[9:12].view(np.int32), pos[[0, 1, 3]].view(np.int32))
    np.testing.assert_array_equal(pts[12:], np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 0], [0, 0.5, 0], [0.5, 0, 0]], np.float32))


def _square(z):
    pos = np.array([[0, 0, z], [1, 0, z], [0, 1, z], [1, 1, z]], np.float32)
    return pos, np.array([[0, 1, 2], [3, 2, 1]], np.int32)


def test_parallel_squares_score_their_distance():
    a, _ = CR.sample_triangles(*_square(0.0), 0.125)
    b, _ = CR.sample_triangles(*_square(0.03125), 0.125)
    assert len(a) == len(b) == 2 * (3 + sum(range(1, 9)))
    q = CR.quality(a, b, 0.05, 0.2)
    assert q["accuracy"] == 0.03125 and q["completion"] == 0.03125 and q["completion_ratio"] == 1.0 and q["precision"] == 1.0
    far = CR.quality(a, b + np.float32(1.0), 0.05, 0.2)              # nothing within r_max: every distance is truncated there
    assert far["accuracy"] == float(np.float32(0.2)) and far["completion_ratio"] == 0.0


def test_nearest_edge_cases():
    t = np.array([[0, 0, 0], [1, 0, 0], [0, 0, 0], [np.nan, 0, 0], [np.inf, 0, 0]], np.float32)
    beyond = np.nextafter(np.float32(0.25), np.float32(1))
    q = np.array([[0.25, 0, 0], [beyond, 0, 0], [0.5, 0, 0], [np.nan, 0, 0], [0, np.inf, 0], [0.875, 0, 0]], np.float32)
    d, i = CR.nearest(q, t, 0.25)
    assert i.tolist() == [0, -1, -1, -1, -1, 1]                     # the lowest of the duplicates; exactly r_max is found
    assert d.tolist() == [0.25, 0.25, 0.25, 0.25, 0.25, 0.125]
    d, i = CR.nearest(q, np.zeros((0, 3), np.float32), 0.25)
    assert (i == -1).all() and (d == 0.25).all()


def test_brute_force_agrees_with_a_kd_tree():
    sp = pytest.importorskip("scipy.spatial")
    rng = np.random.default_rng(5)
    t = rng.random((3000, 3), dtype=np.float32) * np.array([2.0, 1.0, 1.5], np.float32)
    q = rng.random((2000, 3), dtype=np.float32) * np.array([2.0, 1.0, 1.5], np.float32)
    d, i = CR.nearest(q, t, 0.0625)
    dd, ii = sp.cKDTree(t.astype(np.float64)).query(q.astype(np.float64), k=1, distance_upper_bound=0.0625)
    found = np.isfinite(dd)
    assert 200 < found.sum() < 1900
    np.testing.assert_array_equal(i >= 0, found)
    np.testing.assert_array_equal(i[found], ii[found])
    np.testing.assert_allclose(d[found], dd[found], rtol=1e-6, atol=0)


def test_distance_stats_restatement():
    dist = np.array([0.0, 0.04, 0.05, 0.06, 0.2, 0.2], np.float32)
    index = np.array([0, 1, 2, 1, -1, -1], np.int32)
    query = np.zeros((6, 3), np.float32)
    query[5, 1] = np.nan
    counts, sums, conf = CR.distance_stats(dist, index, 0.05, 3, query, np.array([0, 1, 5, 1, 0, 0]), np.array([0, 1, 1]), 2)
    assert counts.tolist() == [5, 4, 3]
    assert sums[0] == pytest.approx(float(dist[:5].astype(np.float64).sum())) and sums[1] == pytest.approx(float(dist[:4].astype(np.float64).sum()))
    assert conf.tolist() == [[1, 0], [0, 1]]                        # the third pair has a query label outside [0, 2)


# ------------------------------------------------------------------ the C ABI without a GPU
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as G
    import apnrf_amd
    G.build()
    return apnrf_amd.load_library()


def _scan(lib, n):
    return int(lib.mnf_scan_workspace_bytes(max(n, 1)))


def _box(*v):
    return (ctypes.c_float * 6)(*v)


def test_workspace_byte_functions(lib):
    """The two layouts of csrc/cloud.hip as the header documents them: 16 B per triangle, 20 B per row (the int32 array padded to 8), two totals
    and the scan's own; 20 B per target and 12 B per query (each array padded to 16), 32 B per cell + 16 (+ padding) and the scan's own."""
    def pad(n, g):
        return (n + g - 1) // g * g
    for T, R in ((0, 0), (1, 1), (3, 7), (300, 4096), (1 << 20, 1 << 24)):
        want = 16 * T + 16 * R + pad(4 * R, 8) + 16 + pad(_scan(lib, max(T, R)), 8)
        assert lib.mnf_cloud_sample_triangles_workspace_bytes(T, R) == want, (T, R)
    for args in ((-1, 0), (0, -1), (1 << 31, 0), (0, 1 << 31)):
        assert lib.mnf_cloud_sample_triangles_workspace_bytes(*args) == 0, args
    # cells: edge = max(r_max (1 + 2^-10), widest / 128); per axis min(128, floor(extent / edge) + 1)
    cases = {(5, 3, (0, 0, 0, 0, 0, 0), 1.0): 1, (4000, 3000, (0, 0, 0, 1.75, 0.75, 1.25), 0.25): 7 * 3 * 5, (10, 10, (0, 0, 0, 1000, 1, 490), 0.5): 128 * 1 * 63,
             (7, 0, (-1, -1, -1, 1, 1, 1), 0.001): 128 ** 3}
    for (n, m, box, r), cells in cases.items():
        want = pad(16 * m, 16) + pad(16 * cells, 16) + 2 * pad(8 * (cells + 1), 16) + pad(4 * m, 16) + 3 * pad(4 * n, 16) + pad(_scan(lib, cells), 16)
        assert lib.mnf_cloud_nearest_workspace_bytes(n, m, _box(*box), r) == want, (n, m, box, r)
    unit = _box(0, 0, 0, 1, 1, 1)
    assert lib.mnf_cloud_nearest_workspace_bytes(-1, 1, unit, 0.5) == 0 and lib.mnf_cloud_nearest_workspace_bytes(1, 1 << 31, unit, 0.5) == 0
    assert lib.mnf_cloud_nearest_workspace_bytes(1, 1, unit, 0.0) == 0 and lib.mnf_cloud_nearest_workspace_bytes(1, 1, unit, float("nan")) == 0
    # r_max * r_max must be a normal float32: 2^-60 is the smallest radius taken
    assert lib.mnf_cloud_nearest_workspace_bytes(1, 1, unit, 2.0 ** -61) == 0 and lib.mnf_cloud_nearest_workspace_bytes(1, 1, unit, 2.0 ** -60) > 0
    assert lib.mnf_cloud_nearest_workspace_bytes(1, 1, _box(0, 0, 0, 1, -1, 1), 0.5) == 0
    assert lib.mnf_cloud_nearest_workspace_bytes(1, 1, _box(0, 0, 0, float("inf"), 1, 1), 0.5) == 0
    assert lib.mnf_cloud_nearest_workspace_bytes(1, 1, None, 0.5) == 0


P = ctypes.c_void_p(1 << 20)        # a well-aligned address that is never touched: every call below is refused before any HIP call
ODD = ctypes.c_void_p((1 << 20) + 4)
BIG = 1 << 40


def _refused(lib, fn, args, what):
    assert fn(*args, None) == -1, what
    assert lib.mnf_last_error().decode(), what


def test_sample_triangles_argument_errors(lib):
    good = dict(positions=P, V=3, triangles=P, T=1, res=0.01, max_rows=8, max_points=8, points=P, face=P, info=P, ws=P, ws_bytes=BIG)
    bad = [dict(V=-1), dict(V=1 << 31), dict(T=-1), dict(T=1 << 31), dict(res=0.0), dict(res=-1.0), dict(res=float("nan")), dict(res=float("inf")),
           dict(max_rows=-1), dict(max_rows=1 << 31), dict(max_points=-1), dict(max_points=1 << 31), dict(positions=None), dict(triangles=None),
           dict(points=None), dict(face=None), dict(info=None), dict(info=ODD), dict(ws=None), dict(ws=ODD), dict(ws_bytes=8)]
    for change in bad:
        _refused(lib, lib.mnf_cloud_sample_triangles, list({**good, **change}.values()), change)


def test_nearest_argument_errors(lib):
    unit = _box(0, 0, 0, 1, 1, 1)
    good = dict(query=P, n=4, target=P, m=4, r_max=0.25, box=unit, index=P, dist=P, ws=P, ws_bytes=BIG)
    bad = [dict(n=-1), dict(n=1 << 31), dict(m=-1), dict(m=1 << 31), dict(r_max=0.0), dict(r_max=-1.0), dict(r_max=float("nan")), dict(r_max=float("inf")),
           dict(r_max=1e30), dict(r_max=2.0 ** -61), dict(r_max=1e-30), dict(box=None), dict(box=_box(0, 0, 0, 1, 1, -1)), dict(box=_box(0, float("nan"), 0, 1, 1, 1)), dict(query=None),
           dict(target=None), dict(index=None), dict(dist=None), dict(ws=None), dict(ws=ODD), dict(ws=ctypes.c_void_p((1 << 20) + 8)), dict(ws_bytes=64)]
    for change in bad:
        _refused(lib, lib.mnf_cloud_nearest, list({**good, **change}.values()), change)


def test_distance_stats_argument_errors(lib):
    good = dict(dist=P, index=P, query=P, n=4, thr=0.05, r_max=0.2, ql=P, tl=P, m=4, C=3, counts=P, sums=P, confusion=P)
    bad = [dict(n=-1), dict(n=1 << 31), dict(m=-1), dict(m=1 << 31), dict(thr=-0.01), dict(thr=0.25), dict(thr=float("nan")), dict(r_max=0.0),
           dict(r_max=float("inf")), dict(dist=None), dict(index=None), dict(counts=None), dict(sums=None), dict(counts=ODD), dict(sums=ODD),
           dict(confusion=ODD), dict(C=0), dict(C=1025), dict(ql=None), dict(tl=None)]
    for change in bad:
        _refused(lib, lib.mnf_cloud_distance_stats, list({**good, **change}.values()), change)


# ------------------------------------------------------------------ the PLY reader
def test_ply_reader_ascii_float_and_double(tmp_path):
    from apnrf_amd.cloud import load_point_cloud_ply
    pts = np.array([[0.5, -1.25, 2.0], [1e-3, 7.0, -0.125], [3.0, 4.0, 5.0]], np.float64)
    rgb = np.array([[255, 0, 7], [1, 2, 3], [9, 8, 200]], np.uint8)
    # ascii with colours and a property to skip, as open3d writes a cloud with normals
    p = tmp_path / "ascii.ply"
    body = "".join(f"{a[0]!r} {a[1]!r} {a[2]!r} 0.0 {c[0]} {c[1]} {c[2]}\n" for a, c in zip(pts.tolist(), rgb.tolist()))
    p.write_text("ply\nformat ascii 1.0\ncomment hand-written\nelement vertex 3\nproperty double x\nproperty double y\nproperty double z\nproperty float quality\n"
                 "property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n" + body)
    got = load_point_cloud_ply(str(p))
    np.testing.assert_array_equal(got["points"], pts.astype(np.float32))
    np.testing.assert_array_equal(got["colour"], rgb)
    # binary little endian, float32, no colours
    p = tmp_path / "float.ply"
    p.write_bytes(b"ply\nformat binary_little_endian 1.0\nelement vertex 3\nproperty float x\nproperty float y\nproperty float z\nend_header\n"
                  + pts.astype("<f4").tobytes())
    got = load_point_cloud_ply(str(p))
    np.testing.assert_array_equal(got["points"], pts.astype(np.float32))
    assert got["colour"] is None and got["points"].dtype == np.float32
    # binary little endian, double with colours and a skipped int, followed by an element that is ignored
    p = tmp_path / "double.ply"
    rec = np.zeros(3, np.dtype([("x", "<f8"), ("y", "<f8"), ("z", "<f8"), ("id", "<i4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")]))
    rec["x"], rec["y"], rec["z"], rec["id"] = pts[:, 0], pts[:, 1], pts[:, 2], [7, 8, 9]
    rec["red"], rec["green"], rec["blue"] = rgb[:, 0], rgb[:, 1], rgb[:, 2]
    p.write_bytes(b"ply\nformat binary_little_endian 1.0\nelement vertex 3\nproperty double x\nproperty double y\nproperty double z\nproperty int id\n"
                  b"property uchar red\nproperty uchar green\nproperty uchar blue\nelement face 0\nproperty list uchar int vertex_indices\nend_header\n"
                  + rec.tobytes())
    got = load_point_cloud_ply(str(p))
    np.testing.assert_array_equal(got["points"], pts.astype(np.float32))
    np.testing.assert_array_equal(got["colour"], rgb)
    # refusals
    p = tmp_path / "big.ply"
    p.write_bytes(b"ply\nformat binary_big_endian 1.0\nelement vertex 0\nproperty float x\nproperty float y\nproperty float z\nend_header\n")
    with pytest.raises(ValueError):
        load_point_cloud_ply(str(p))
    p = tmp_path / "short.ply"
    p.write_bytes(b"ply\nformat binary_little_endian 1.0\nelement vertex 3\nproperty float x\nproperty float y\nproperty float z\nend_header\n" + b"\0" * 35)
    with pytest.raises(ValueError):
        load_point_cloud_ply(str(p))
