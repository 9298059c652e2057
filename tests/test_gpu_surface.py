"""GPU tests of the surface mesh (csrc/surface.hip, apnrf_amd/surface.py) against the numpy restatement tests/surface_ref.py, which
tests/test_surface_cpu.py holds to the definition.  Every comparison is `array_equal` on counts, `info`, the bits of positions and normals,
triangle indices, colours and labels; only `measure` has a tolerance, the bound of any summation order.  Outputs of the C ABI are
allocated with guard elements on both sides."""
import ctypes
import math

import numpy as np
import pytest
import torch

import surface_ref as SR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64
MARK32, MARK64, MARK8 = -0x5A5A5A5B, -0x5A5A5A5A5A5A5A5B, 0xA5


def _dev(a):
    return torch.from_numpy(np.array(a, copy=True, order="C")).to(DEV)


def _guarded(n, dtype, mark):
    whole = torch.full((n + 2 * GUARD,), mark, dtype=dtype, device=DEV)
    return whole, whole[GUARD:GUARD + n]


def _assert_guards(whole, n, mark, what):
    host = whole.cpu().numpy()
    assert (host[:GUARD] == mark).all() and (host[GUARD + n:] == mark).all(), f"{what}: written outside its bounds"


def _f3(v):
    return (ctypes.c_float * 3)(*[float(np.float32(x)) for x in v])


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


# ------------------------------------------------------------------ the lattices and their reference meshes, computed once
FRAME = ((0.5, -1.25, 2.0), (0.25, 0.5, 0.125))                     # origin, step: anisotropic, exact in float32


def _special(kind):
    v = SR.ball((9, 9, 9), 2.6)
    if kind == "on_iso":
        v[4, 4, 4] = np.float32(0.25)
    else:
        v[4, 4, 4] = v[1, 1, 1] = {"nan": np.nan, "inf": np.inf, "ninf": -np.inf}[kind]
        v[8, 8, 8] = v[4, 4, 4]                                     # and one on the boundary: one-sided differences meet it
    return v


LATTICES = {
    "point": (SR.single_point, 0.5),
    "ball9": (lambda: SR.ball((9, 9, 9), 2.6), 0.0),
    "ball_odd": (lambda: SR.ball((17, 13, 11), 3.9), 0.0),
    "torus_odd": (lambda: SR.torus((17, 13, 11), 3.2, 1.4), 0.0),
    "ball33": (lambda: SR.ball((33, 33, 33), 11.7), 0.0),
    "sliver": (lambda: np.array([[[1.0, -1.0], [-3.0, -1.0]], [[-1.0, -2.0], [-1.0, -1.0]], [[-1.0, -1.0], [-1.0, 5.0]]], np.float32), 0.0),
    "nan": (lambda: _special("nan"), 0.25),
    "inf": (lambda: _special("inf"), 0.25),
    "ninf": (lambda: _special("ninf"), 0.25),
    "on_iso": (lambda: _special("on_iso"), 0.25),
    "slab": (lambda: np.where((np.arange(7) // 2 == 1)[:, None, None], np.float32(1), np.float32(-1)) * np.ones((7, 6, 9), np.float32), 0.0),
}
_REF = {}


def reference(name):
    if name not in _REF:
        make, iso = LATTICES[name]
        values = np.ascontiguousarray(make(), np.float32)
        m = SR.extract(values, iso, *FRAME)
        values.setflags(write=False)
        for k in ("positions", "normals", "triangles"):
            m[k].setflags(write=False)
        _REF[name] = (values, iso, m)
    return _REF[name]


def gpu_extract(values, iso, max_v, max_t, frame=FRAME):
    """mnf_surface_extract through the C ABI -> (positions bits [max_v,3], normals bits, triangles [max_t,3], info [4]) as the call left them."""
    from apnrf_amd import _lib as L
    lib = L.load_library()
    cells = tuple(n - 1 for n in values.shape)
    nbytes = int(lib.mnf_surface_extract_workspace_bytes(*cells))
    assert nbytes >= values.size * 4
    pw, pos = _guarded(3 * max_v, torch.int32, MARK32)
    nw, nrm = _guarded(3 * max_v, torch.int32, MARK32)
    tw, tri = _guarded(3 * max_t, torch.int32, MARK32)
    iw, info = _guarded(4, torch.int64, MARK64)
    ww, ws = _guarded(nbytes // 8, torch.int64, MARK64)
    d_v = _dev(values)
    L.launch(lib.mnf_surface_extract, L.ptr(d_v), *cells, float(iso), _f3(frame[0]), _f3(frame[1]), max_v, max_t, L.ptr(pos) if max_v else None,
             L.ptr(nrm) if max_v else None, L.ptr(tri) if max_t else None, L.ptr(info), L.ptr(ws), nbytes, device=torch.device(DEV))
    torch.cuda.synchronize()
    for whole, n, mark, what in ((pw, 3 * max_v, MARK32, "positions"), (nw, 3 * max_v, MARK32, "normals"), (tw, 3 * max_t, MARK32, "triangles"),
                                 (iw, 4, MARK64, "info"), (ww, nbytes // 8, MARK64, "workspace")):
        _assert_guards(whole, n, mark, what)
    return pos.cpu().numpy().reshape(max_v, 3), nrm.cpu().numpy().reshape(max_v, 3), tri.cpu().numpy().reshape(max_t, 3), info.cpu().numpy()


# ------------------------------------------------------------------ the surface of a lattice, bit for bit
@pytest.mark.parametrize("name", list(LATTICES))
def test_extract_matches_the_restatement(name):
    values, iso, m = reference(name)
    V, T = len(m["positions"]), len(m["triangles"])
    assert V > 0 and T > 0
    pos, nrm, tri, info = gpu_extract(values, iso, V, T)
    assert info.tolist() == [V, T, 0, 0]
    np.testing.assert_array_equal(pos, _bits(m["positions"]))
    np.testing.assert_array_equal(nrm, _bits(m["normals"]))
    np.testing.assert_array_equal(tri, m["triangles"])
    # a counting call, and roomy capacities: the counts stay, the rest of the buffers is left alone
    assert gpu_extract(values, iso, 0, 0)[3].tolist() == [V, T, V, T]
    pos2, _, tri2, info2 = gpu_extract(values, iso, V + 5, T + 3)
    assert info2.tolist() == [V, T, 0, 0] and (pos2[V:] == MARK32).all() and (tri2[T:] == MARK32).all()
    np.testing.assert_array_equal(pos2[:V], pos)
    np.testing.assert_array_equal(tri2[:T], tri)


def test_empty_surfaces():
    for v in (np.zeros((3, 4, 2), np.float32), np.ones((3, 4, 2), np.float32), np.full((2, 2, 2), np.nan, np.float32)):
        pos, _, tri, info = gpu_extract(v, 0.5, 4, 4)
        assert info.tolist() == [0, 0, 0, 0] and (pos == MARK32).all() and (tri == MARK32).all()


@pytest.mark.parametrize("short_v,short_t", [(1, 0), (0, 1), (1, 1)])
def test_capacities_one_short(short_v, short_t):
    values, iso, m = reference("torus_odd")
    V, T = len(m["positions"]), len(m["triangles"])
    mv, mt = V - short_v, T - short_t
    pos, nrm, tri, info = gpu_extract(values, iso, mv, mt)          # the guards around every buffer are checked in there
    assert info.tolist() == [V, T, short_v, short_t]
    np.testing.assert_array_equal(pos, _bits(m["positions"])[:mv])
    np.testing.assert_array_equal(nrm, _bits(m["normals"])[:mv])
    want = m["triangles"][:mt].copy()
    beyond = (want >= mv).any(axis=1)                               # a triangle that names a vertex beyond the capacity: counted, not written
    assert beyond.any() == bool(short_v)
    want[beyond] = MARK32
    np.testing.assert_array_equal(tri, want)


def test_measure_within_the_bound_of_any_summation_order():
    from apnrf_amd import _lib as L
    for name in ("point", "ball33", "torus_odd"):
        values, iso, m = reference(name)
        V, T = len(m["positions"]), len(m["triangles"])
        area_t, vol_t = SR.measure_terms(m["positions"], m["triangles"])
        ow, out = _guarded(2, torch.float64, -1.5)
        info = _dev(np.array([V, T, 0, 0], np.int64))
        # capacities larger than the counts, garbage behind them: the counts are read on the device
        pos = torch.cat([_dev(m["positions"]), torch.full((7, 3), 1e30, device=DEV)])
        tri = torch.cat([_dev(m["triangles"]), torch.zeros(5, 3, dtype=torch.int32, device=DEV)])
        L.launch(L.load_library().mnf_surface_measure, L.ptr(pos), L.ptr(tri), L.ptr(info), V + 7, T + 5, L.ptr(out))
        torch.cuda.synchronize()
        _assert_guards(ow, 2, -1.5, "measure")
        got = out.cpu().numpy()
        for g, terms in ((got[0], area_t), (got[1], vol_t)):
            bound = T * 2.0 ** -52 * math.fsum(np.abs(terms).tolist())
            err = abs(float(g) - math.fsum(terms.tolist()))
            print(f"{name}: measure {float(g)!r}, error {err:.3e}, bound {bound:.3e}")
            assert err <= bound
        assert got[1] > 0.0                                          # outward orientation: every one of these meshes is closed


# ------------------------------------------------------------------ the module
def test_module_extract_and_overflow():
    from apnrf_amd import _lib as L
    from apnrf_amd.surface import extract_lattice_surface
    values, iso, m = reference("ball_odd")
    V, T = len(m["positions"]), len(m["triangles"])
    mesh = extract_lattice_surface(_dev(values), iso, *FRAME)
    assert mesh.positions.dtype == torch.float32 and mesh.triangles.dtype == torch.int32 and mesh.positions.is_cuda
    assert (mesh.n_vertices, mesh.n_triangles) == (V, T) and mesh.info.cpu().tolist() == [V, T, 0, 0]
    np.testing.assert_array_equal(_bits(mesh.positions.cpu().numpy()), _bits(m["positions"]))
    np.testing.assert_array_equal(_bits(mesh.normals.cpu().numpy()), _bits(m["normals"]))
    np.testing.assert_array_equal(mesh.triangles.cpu().numpy(), m["triangles"])
    area, volume = SR.measure(m["positions"], m["triangles"])
    got = mesh.measure()
    assert abs(got["area"] - area) <= 1e-9 * area and abs(got["volume"] - volume) <= 1e-9 * abs(volume)
    roomy = extract_lattice_surface(_dev(values), iso, *FRAME, max_vertices=V + 9, max_triangles=T)
    assert roomy.n_vertices == V and roomy.n_triangles == T
    with pytest.raises(L.MnfError, match=rf"{V} vertices.*max_vertices = {V - 1}"):
        extract_lattice_surface(_dev(values), iso, *FRAME, max_vertices=V - 1, max_triangles=T)
    with pytest.raises(L.MnfError, match=rf"{T} triangles.*max_triangles = {T - 1}"):
        extract_lattice_surface(_dev(values), iso, *FRAME, max_triangles=T - 1)
    host = mesh.cpu()
    assert not host.positions.is_cuda and host.colour is None


# ------------------------------------------------------------------ lattice points
def _hand_made_binaries():
    b = np.zeros((4, 3, 5), bool)
    b[0, 0, 0] = True                                               # a corner
    b[2, 1, 2] = True                                               # the middle
    return b


def gpu_lattice_points(binaries, refine, aabb, cap):
    from apnrf_amd import _lib as L
    lib = L.load_library()
    R = binaries.shape
    nbytes = int(lib.mnf_surface_lattice_points_workspace_bytes(*R, refine))
    assert nbytes > 0 and nbytes % 8 == 0
    lw, lin = _guarded(cap, torch.int32, MARK32)
    pw, pos = _guarded(3 * cap, torch.int32, MARK32)
    iw, info = _guarded(2, torch.int64, MARK64)
    ww, ws = _guarded(nbytes // 8, torch.int64, MARK64)
    d_b = _dev(binaries.astype(np.uint8))
    L.launch(lib.mnf_surface_lattice_points, L.ptr(d_b), *R, refine, (ctypes.c_float * 6)(*[float(np.float32(x)) for x in aabb]), cap,
             L.ptr(lin) if cap else None, L.ptr(pos) if cap else None, L.ptr(info), L.ptr(ws), nbytes, device=torch.device(DEV))
    torch.cuda.synchronize()
    for whole, n, mark, what in ((lw, cap, MARK32, "lin"), (pw, 3 * cap, MARK32, "positions"), (iw, 2, MARK64, "info"), (ww, nbytes // 8, MARK64, "workspace")):
        _assert_guards(whole, n, mark, what)
    return lin.cpu().numpy(), pos.cpu().numpy().reshape(cap, 3), info.cpu().numpy()


@pytest.mark.parametrize("refine", [1, 2])
def test_lattice_points(refine):
    b = _hand_made_binaries()
    aabb = (-1.0, 0.5, 2.0, 1.4, 1.7, 4.5)
    lin_r, pos_r, _, _, shape = SR.lattice_points(b, refine, aabb)
    n = len(lin_r)
    assert 0 < n < shape[0] * shape[1] * shape[2]
    lin, pos, info = gpu_lattice_points(b, refine, aabb, n)
    assert info.tolist() == [n, 0]
    np.testing.assert_array_equal(lin, lin_r)
    np.testing.assert_array_equal(pos, _bits(pos_r))
    lin, pos, info = gpu_lattice_points(b, refine, aabb, n - 1)       # one short
    assert info.tolist() == [n, 1]
    np.testing.assert_array_equal(lin, lin_r[:-1])
    np.testing.assert_array_equal(pos, _bits(pos_r)[:-1])
    assert gpu_lattice_points(b, refine, aabb, 0)[2].tolist() == [n, n]
    lin, _, info = gpu_lattice_points(np.zeros_like(b), refine, aabb, 8)  # an empty grid
    assert info.tolist() == [0, 0] and (lin == MARK32).all()
    full = np.ones_like(b)
    lin, _, info = gpu_lattice_points(full, refine, aabb, int(np.prod(shape)))
    assert info.tolist() == [int(np.prod(shape)), 0] and np.array_equal(lin, np.arange(np.prod(shape)))


def test_lattice_scatter():
    from apnrf_amd import _lib as L
    n_values = 700
    vw, values = _guarded(n_values, torch.float32, 7.5)
    lin = _dev(np.array([3, 699, 0, 41, 5], np.int32))
    dens = _dev(np.array([1.5, 2.5, 3.5, 4.5, 99.0], np.float32))
    info = _dev(np.array([4, 0], np.int64))                          # the fifth entry is past the count
    L.launch(L.load_library().mnf_surface_lattice_scatter, L.ptr(dens), L.ptr(lin), L.ptr(info), 5, L.ptr(values), n_values)
    torch.cuda.synchronize()
    _assert_guards(vw, n_values, 7.5, "values")
    want = np.zeros(n_values, np.float32)
    want[[3, 699, 0, 41]] = [1.5, 2.5, 3.5, 4.5]
    np.testing.assert_array_equal(values.cpu().numpy(), want)


# ------------------------------------------------------------------ vertex attributes
def test_vertex_attrs():
    from apnrf_amd import _lib as L
    rng = np.random.default_rng(5)
    n, C = 1000, 29
    rgb = rng.uniform(-0.2, 1.2, (n, 3)).astype(np.float32)
    rgb[:6] = [[0.0, 1.0, 0.5], [np.nan, 0.25, 0.75], [np.inf, -np.inf, 1e-9], [0.5 / 255, 1.5 / 255, 254.5 / 255], [0.49999 / 255, 0.998, 0.002], [-0.0, 2.0, 0.999]]
    sem = rng.normal(size=(n, C)).astype(np.float32)
    sem[0, 3] = sem[0, 17] = 9.0                                    # a tie: the first index
    sem[1, 11] = np.nan
    sem[2, 28] = np.inf
    sem[3] = -np.inf
    sem[4] = 0.0
    palette = rng.integers(0, 256, (C, 3)).astype(np.uint8)
    want = SR.vertex_attrs(rgb, sem, palette)
    assert want["label"][:5].tolist() == [3, -1, 28, 0, 0]
    cw, colour = _guarded(3 * n, torch.uint8, MARK8)
    lw, label = _guarded(n, torch.int32, MARK32)
    sw, semc = _guarded(3 * n, torch.uint8, MARK8)
    d_rgb, d_sem, d_pal = _dev(rgb), _dev(sem), _dev(palette)
    L.launch(L.load_library().mnf_surface_vertex_attrs, L.ptr(d_rgb), L.ptr(d_sem), n, C, L.ptr(d_pal), L.ptr(colour), L.ptr(label), L.ptr(semc))
    torch.cuda.synchronize()
    for whole, k, mark, what in ((cw, 3 * n, MARK8, "colour"), (lw, n, MARK32, "label"), (sw, 3 * n, MARK8, "sem_colour")):
        _assert_guards(whole, k, mark, what)
    np.testing.assert_array_equal(colour.cpu().numpy().reshape(n, 3), want["colour"])
    np.testing.assert_array_equal(label.cpu().numpy(), want["label"])
    np.testing.assert_array_equal(semc.cpu().numpy().reshape(n, 3), want["sem_colour"])
    from apnrf_amd.surface import vertex_attrs
    a = vertex_attrs(d_rgb, d_sem)
    assert "sem_colour" not in a and a["colour"].dtype == torch.uint8 and a["label"].dtype == torch.int32
    np.testing.assert_array_equal(a["colour"].cpu().numpy(), want["colour"])
    np.testing.assert_array_equal(a["label"].cpu().numpy(), want["label"])


# ------------------------------------------------------------------ end to end
def test_field_to_mesh(tmp_path):
    import helpers as H
    from apnrf_amd import surface as SF
    scene = H.make_scene(log2_hashmap_size=15)
    field, est = H.hip_field(scene), H.hip_estimator(scene)
    R = tuple(est.binaries.shape[1:])
    b = np.zeros((1,) + R, bool)
    b[0, 0, 0, 0] = True
    b[0, R[0] // 2:R[0] // 2 + 2, R[1] // 2, R[2] // 3] = True
    est.binaries = torch.from_numpy(b).to(DEV)
    refine = 2
    aabb = est.aabbs[0].cpu().numpy()
    lin_r, pos_r, origin_r, step_r, shape = SR.lattice_points(b[0], refine, aabb)
    values, origin, step = SF.lattice_from_field(field, est, refine)
    assert tuple(values.shape) == shape and values.dtype == torch.float32
    np.testing.assert_array_equal(_bits(origin), _bits(origin_r))
    np.testing.assert_array_equal(_bits(step), _bits(step_r))
    pts = SF.lattice_points(est.binaries[0], refine, aabb)
    np.testing.assert_array_equal(pts["lin"].cpu().numpy(), lin_r)
    np.testing.assert_array_equal(_bits(pts["positions"].cpu().numpy()), _bits(pos_r))
    density = field.query_density(_dev(pos_r)).reshape(-1).cpu().numpy()
    want = np.zeros(int(np.prod(shape)), np.float32)
    want[lin_r] = density
    host = values.cpu().numpy()
    np.testing.assert_array_equal(_bits(host.reshape(-1)), _bits(want))                # the field's densities where listed, 0 elsewhere
    iso = float(np.median(density))
    assert iso > 0 and np.isfinite(density).all()
    palette = np.random.default_rng(2).integers(0, 256, (scene["C"], 3)).astype(np.uint8)
    mesh = SF.extract_surface(field, est, iso, refine=refine, palette=palette)
    m = SR.extract(host, iso, origin_r, step_r)
    V, T = len(m["positions"]), len(m["triangles"])
    assert V > 100 and T > 100 and (mesh.n_vertices, mesh.n_triangles) == (V, T)
    np.testing.assert_array_equal(_bits(mesh.positions.cpu().numpy()), _bits(m["positions"]))
    np.testing.assert_array_equal(_bits(mesh.normals.cpu().numpy()), _bits(m["normals"]))
    np.testing.assert_array_equal(mesh.triangles.cpu().numpy(), m["triangles"])
    with torch.no_grad():
        rgb, _, sem = field.forward(mesh.positions, -mesh.normals)
    a = SR.vertex_attrs(rgb.cpu().numpy(), sem.cpu().numpy(), palette)
    np.testing.assert_array_equal(mesh.colour.cpu().numpy(), a["colour"])
    np.testing.assert_array_equal(mesh.label.cpu().numpy(), a["label"])
    np.testing.assert_array_equal(mesh.sem_colour.cpu().numpy(), a["sem_colour"])
    assert len(np.unique(a["label"])) > 1 and a["colour"].std() > 0
    path = str(tmp_path / "field.ply")
    mesh.save_ply(path)
    got = SF.load_ply(path)
    for k, w in (("positions", m["positions"]), ("normals", m["normals"]), ("triangles", m["triangles"]), ("colour", a["colour"]), ("label", a["label"])):
        assert got[k].tobytes() == np.ascontiguousarray(w).tobytes(), k


@pytest.mark.parametrize("why", ["empty_grid", "iso_above_every_density"])
def test_field_to_an_empty_mesh(tmp_path, why):
    """No occupied cell yet, or an iso above every evaluated density: the whole route returns a mesh of nothing, and every method of it works."""
    import helpers as H
    from apnrf_amd import surface as SF
    scene = H.make_scene(log2_hashmap_size=15)
    field, est = H.hip_field(scene), H.hip_estimator(scene)
    R = tuple(est.binaries.shape[1:])
    b = np.zeros((1,) + R, bool)
    iso = 10.0
    if why == "iso_above_every_density":
        b[0, R[0] // 2, R[1] // 2, R[2] // 3] = True
        iso = 3.0e38
    est.binaries = torch.from_numpy(b).to(DEV)
    values, _, _ = SF.lattice_from_field(field, est, 1)
    assert bool((values != 0).any()) == (why != "empty_grid") and float(values.max()) < iso
    palette = np.arange(3 * scene["C"], dtype=np.uint8).reshape(-1, 3)
    mesh = SF.extract_surface(field, est, iso, refine=1, palette=palette)
    assert (mesh.n_vertices, mesh.n_triangles) == (0, 0) and mesh.info.cpu().tolist() == [0, 0, 0, 0]
    for t, shape, dtype in ((mesh.positions, (0, 3), torch.float32), (mesh.normals, (0, 3), torch.float32), (mesh.triangles, (0, 3), torch.int32),
                            (mesh.colour, (0, 3), torch.uint8), (mesh.label, (0,), torch.int32), (mesh.sem_colour, (0, 3), torch.uint8)):
        assert tuple(t.shape) == shape and t.dtype == dtype and t.is_cuda
    assert mesh.measure() == {"area": 0.0, "volume": 0.0}
    path = str(tmp_path / "empty.ply")
    mesh.save_ply(path)
    got = SF.load_ply(path)
    assert got["positions"].shape == (0, 3) and got["normals"].shape == (0, 3) and got["colour"].shape == (0, 3)
    assert got["label"].shape == (0,) and got["triangles"].shape == (0, 3) and got["triangles"].dtype == np.int32
    # the attributes alone, of no vertex, with and without a palette
    a = SF.vertex_attrs(torch.empty(0, 3, device=DEV), torch.empty(0, scene["C"], device=DEV))
    assert tuple(a["colour"].shape) == (0, 3) and tuple(a["label"].shape) == (0,) and "sem_colour" not in a
    a = SF.vertex_attrs(torch.empty(0, 3, device=DEV), torch.empty(0, scene["C"], device=DEV), torch.from_numpy(palette).to(DEV))
    assert tuple(a["sem_colour"].shape) == (0, 3) and a["sem_colour"].dtype == torch.uint8


# ------------------------------------------------------------------ argument errors: refused before any HIP call
def test_argument_errors():
    from apnrf_amd import _lib as L
    lib = L.load_library()
    values = torch.zeros(3, 3, 3, dtype=torch.float32, device=DEV)
    nbytes = int(lib.mnf_surface_extract_workspace_bytes(2, 2, 2))
    ws = torch.zeros(nbytes // 8 + 1, dtype=torch.int64, device=DEV)
    out = torch.zeros(64, dtype=torch.int64, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    o, s = _f3((0, 0, 0)), _f3((1, 1, 1))

    def extract(values=p(values), cells=(2, 2, 2), iso=0.5, origin=o, step=s, mv=4, mt=4, pos=p(out), nrm=p(out), tri=p(out), info=p(out), w=p(ws), wb=nbytes):
        return lib.mnf_surface_extract(values, *cells, iso, origin, step, mv, mt, pos, nrm, tri, info, w, wb, None)

    bad = [dict(values=None), dict(pos=None), dict(nrm=None), dict(tri=None), dict(info=None), dict(w=None), dict(origin=None), dict(step=None),
           dict(cells=(0, 2, 2)), dict(cells=(2, 1025, 2)), dict(cells=(2, 2, -1)), dict(step=_f3((1, 0, 1))), dict(step=_f3((1, 1, -2))),
           dict(step=_f3((np.inf, 1, 1))), dict(step=_f3((1, np.nan, 1))), dict(iso=float("nan")), dict(iso=float("inf")), dict(mv=-1), dict(mt=-1),
           dict(mv=1 << 31), dict(w=ctypes.c_void_p(ws.data_ptr() + 4)), dict(wb=nbytes - 1), dict(info=ctypes.c_void_p(out.data_ptr() + 4))]
    for kw in bad:
        assert extract(**kw) == -1, kw
        assert lib.mnf_last_error()
    assert lib.mnf_surface_extract_workspace_bytes(0, 1, 1) == 0 and lib.mnf_surface_extract_workspace_bytes(1, 1, 1025) == 0
    assert lib.mnf_surface_extract_workspace_bytes(1024, 1024, 1024) > 4 * 1025 ** 3
    # measure
    assert lib.mnf_surface_measure(None, p(out), p(out), 4, 4, p(out), None) == -1
    assert lib.mnf_surface_measure(p(out), None, p(out), 4, 4, p(out), None) == -1
    assert lib.mnf_surface_measure(p(out), p(out), None, 4, 4, p(out), None) == -1
    assert lib.mnf_surface_measure(p(out), p(out), p(out), 4, 4, None, None) == -1
    assert lib.mnf_surface_measure(p(out), p(out), p(out), -1, 4, p(out), None) == -1
    assert lib.mnf_surface_measure(p(out), p(out), p(out), 4, -1, p(out), None) == -1
    # lattice points
    aabb = (ctypes.c_float * 6)(0, 0, 0, 1, 1, 1)
    pb = int(lib.mnf_surface_lattice_points_workspace_bytes(4, 3, 5, 2))

    def points(b=p(out), R=(4, 3, 5), refine=2, aabb=aabb, cap=4, lin=p(out), pos=p(out), info=p(out), w=None, wb=pb):
        return lib.mnf_surface_lattice_points(b, *R, refine, aabb, cap, lin, pos, info, w, wb, None)

    assert pb > 0
    ws_big = torch.zeros(pb // 8 + 1, dtype=torch.int64, device=DEV)
    for kw in [dict(b=None), dict(lin=None), dict(pos=None), dict(info=None), dict(w=None), dict(aabb=None), dict(refine=3), dict(refine=0), dict(refine=16),
               dict(R=(0, 3, 5)), dict(R=(4, 3, 513)), dict(R=(4, 1025, 5), refine=1), dict(cap=-1), dict(aabb=(ctypes.c_float * 6)(0, 0, 0, 1, 0, 1)),
               dict(aabb=(ctypes.c_float * 6)(0, 0, 0, 1, float("inf"), 1)), dict(w=ctypes.c_void_p(ws_big.data_ptr() + 4)), dict(wb=pb - 1)]:
        if "w" not in kw:
            kw["w"] = p(ws_big)
        assert points(**kw) == -1, kw
    assert lib.mnf_surface_lattice_points_workspace_bytes(4, 3, 5, 3) == 0 and lib.mnf_surface_lattice_points_workspace_bytes(129, 3, 5, 8) == 0
    # scatter and attributes
    assert lib.mnf_surface_lattice_scatter(None, p(out), p(out), 4, p(out), 8, None) == -1
    assert lib.mnf_surface_lattice_scatter(p(out), None, p(out), 4, p(out), 8, None) == -1
    assert lib.mnf_surface_lattice_scatter(p(out), p(out), None, 4, p(out), 8, None) == -1
    assert lib.mnf_surface_lattice_scatter(p(out), p(out), p(out), 4, None, 8, None) == -1
    assert lib.mnf_surface_lattice_scatter(p(out), p(out), p(out), -1, p(out), 8, None) == -1
    assert lib.mnf_surface_lattice_scatter(p(out), p(out), p(out), 4, p(out), 0, None) == -1
    assert lib.mnf_surface_vertex_attrs(None, p(out), 4, 3, None, p(out), None, None, None) == -1
    assert lib.mnf_surface_vertex_attrs(p(out), None, 4, 3, None, None, p(out), None, None) == -1
    assert lib.mnf_surface_vertex_attrs(p(out), p(out), 4, 3, None, None, None, p(out), None) == -1      # sem_colour without a palette
    assert lib.mnf_surface_vertex_attrs(p(out), p(out), -1, 3, None, p(out), None, None, None) == -1
    assert lib.mnf_surface_vertex_attrs(p(out), p(out), 4, 0, None, p(out), None, None, None) == -1
    torch.cuda.synchronize()
    assert (out == 0).all() and (ws == 0).all()                       # nothing ran
