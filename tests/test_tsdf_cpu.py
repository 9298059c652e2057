"""tests/tsdf_ref.py, the numpy restatement of TSDF fusion (include/mi355nerf.h "TSDF fusion of captures"), held to things it shares no code
with: the closed form of a wall seen head on, the geometry of a closed room (every point the volume calls inside lies near matter), the
rules of the observed-only extraction, and a vectorised search for the vertex attributes.  No GPU."""
import functools

import numpy as np

import sensor_ref as SR
import surface_ref as SF
import tsdf_ref as T

S = T.S


# ------------------------------------------------------------------ a wall seen head on
def test_wall_matches_the_closed_form():
    """A wall of voxels with its face at x_wall = 12 s, a camera at x = 0.13 looking along +x, planar depth.  Every ray that hits the face
    has planar depth x_wall - x_cam whatever its pixel, so for EVERY observed point, not only those on the optical axis's rows (which are
    checked by themselves too), sdf = x_wall - x_p and one observation leaves tsdf = (float)min(1, sdf / trunc).

    THE BOUND.  The sensor's t_hit is ((12 - g) * inv) with g, inv two float64 roundings each of relative 2^-53, and the restatement's
    zd, sdf and quotient add three more on numbers below 1 m: below 8 * 2^-53 m = 1e-15 m in all.  The depth is stored as float32:
    |d32 - d| <= 2^-24 d.  The tsdf is stored as float32: 2^-24 |s| <= 2^-24 more.  So
        |tsdf - clamp| <= (2^-24 d + 1e-15) / trunc + 2^-24.
    A vertex sits where the line through two such values crosses 0; the exact values are linear in x and cross at x_wall, the errors of
    the two ends enter as a convex combination, so the crossing moves by at most trunc times the bound; the float32 chain of the vertex
    (t: three roundings; (p + t d) step + origin: four, on numbers below 16 voxels = 0.8 m) adds at most 8 * 2^-24 * 0.8 m."""
    shape = (16, 11, 11)
    vox = np.full(shape, 0xFF000000, np.uint32)
    vox[12:] = SR.pack(10, 200, 30, 7)
    lo = np.zeros(3)
    cam = np.array([0.13, 5 * S, 5 * S])                                      # on the lattice rows y = 5, z = 5
    c2w = T.yaw_pose(cam, -90.0)[None]                                       # -R[:, 2] = +x
    assert np.allclose(-c2w[0, :, 2], [1, 0, 0])
    Wp, Hp, f = 24, 20, 12.0
    out = SR.views(vox, lo, S, c2w, Wp, Hp, f, 0.0, 100.0)
    trunc = 4 * S
    vol = T.integrate(T.Volume(shape, lo, S, trunc), c2w, f, out["depth"], out["rgba"], out["sem"], T.PLANAR)
    x_wall = 12 * S
    d = x_wall - cam[0]
    bound = (2.0 ** -24 * d + 1e-15) / trunc + 2.0 ** -24
    xs = np.arange(17) * S
    want = np.minimum(1.0, (x_wall - xs) / trunc)
    obs = vol.weight > 0
    assert obs[3:16, 5, 5].all() and not obs[:3, 5, 5].any() and not obs[16, 5, 5], "the axis row: in front of the camera up to trunc behind the face"
    err_axis = np.abs(vol.tsdf[:, 5, 5].astype(np.float64) - want)[obs[:, 5, 5]].max()
    err_all = np.abs(vol.tsdf.astype(np.float64) - want[:, None, None])[obs].max()
    print(f"wall: tsdf error on the axis row {err_axis:.3e}, over all {int(obs.sum())} observed points {err_all:.3e}, bound {bound:.3e}")
    assert err_axis <= bound and err_all <= bound
    assert (vol.weight[obs] == 1).all() and vol.info.tolist()[0] == int(obs.sum()) == vol.info.tolist()[1] and vol.info[3] > 0
    worded = vol.best >= 0
    assert worded.any() and (vol.word[worded] == SR.pack(*[(c * 200 + 127) // 255 for c in (10, 200, 30)], 7)).all()      # face 0 is shaded with 200
    values, _ = T.lattice(vol)
    mesh = T.extract_observed(values, 0.0, lo.astype(np.float32), np.full(3, S, np.float32))
    assert len(mesh["positions"]) > 20 and len(mesh["triangles"]) > 20
    err_v = np.abs(mesh["positions"][:, 0].astype(np.float64) - x_wall).max()
    print(f"wall: vertices off the face by at most {err_v:.3e}, bound {bound * trunc + 8 * 2.0 ** -24 * 0.8:.3e}")
    assert err_v <= bound * trunc + 8 * 2.0 ** -24 * 0.8


# ------------------------------------------------------------------ the closed room
@functools.lru_cache(maxsize=None)
def _room_volume(mode, repeats=0, max_weight=64):
    c2w, depth, rgba, sem = T.room_captures(mode, repeats)
    vol = T.integrate(T.Volume(T.ROOM_SHAPE, T.ROOM_LO, S, 4 * S, max_weight=max_weight), c2w, T.FOCAL, depth, rgba, sem, mode)
    return vol, c2w


def _box_distance(points, vox):
    """Distance of each point to the nearest occupied voxel's box."""
    idx = np.argwhere(SR.occupied(vox)).astype(np.float64)
    lo, hi = T.ROOM_LO + idx * S, T.ROOM_LO + (idx + 1) * S
    out = np.empty(len(points))
    for i, p in enumerate(points):
        gap = np.maximum(np.maximum(lo - p, p - hi), 0.0)
        out[i] = np.sqrt((gap * gap).sum(axis=1)).min()
    return out


def test_room_counters_and_the_weight_cap():
    """The fixture: the (19, 9, 21) clutter grid at 0.05 m, all six boundary layers occupied, a 5 x 3 x 5 pocket freed at the centre; four
    views at the centre turned 0, 90, 180 and -73 degrees and one looking away from 5 m outside, 24 x 20 pixels at focal 12, four planted
    depths in view 1.  This restatement observes 3455 (planar) and 3335 (ray) of the 4400 points and skips 11 invalid depths and 306 / 450
    observations behind the surface; a throw-away run with a pocket and planted pixels of its own, not recorded, gave 3461, 9 and 281 /
    442.  What is held here does not come from the code under test: every skip rule is exercised, the view that misses counts nothing,
    and the cap binds."""
    for mode in (T.PLANAR, T.RAY):
        vol, c2w = _room_volume(mode)
        observed = int((vol.weight > 0).sum())
        print(f"room, mode {mode}: {observed} of {vol.weight.size} observed, info {vol.info.tolist()}")
        assert vol.weight.size == 4400 and observed > 3000
        assert vol.info[0] == vol.weight.sum() and vol.info[1] == observed, "below the cap every observation is one unit of weight"
        assert vol.info[2] > 0 and vol.info[3] > 0, "invalid depths and behind-surface skips are exercised"
        assert vol.weight.max() < 64
        # the view from outside alone: nothing changes, nothing is counted
        c2w5, depth, rgba, sem = T.room_captures(mode)
        alone = T.integrate(T.Volume(T.ROOM_SHAPE, T.ROOM_LO, S, 4 * S), c2w5[4:5], T.FOCAL, depth[4:5], rgba[4:5], sem[4:5], mode)
        assert alone.info.tolist() == [0] * 5 and (alone.weight == 0).all() and (alone.tsdf == 1).all() and (alone.best == -1).all()
        # an int64 class outside [0, 255] is stored as 255 and counted
        sem64 = sem.astype(np.int64)
        sem64[0] = 300
        big = T.integrate(T.Volume(T.ROOM_SHAPE, T.ROOM_LO, S, 4 * S), c2w5, T.FOCAL, depth, rgba, sem64, mode)
        assert big.info[4] > 0 and ((big.word >> 24)[big.best >= 0] == 255).sum() > 0 and np.array_equal(big.tsdf, vol.tsdf)
        # two repeats of view 0 and max_weight = 3
        capped, _ = _room_volume(mode, 2, 3)
        assert capped.weight.max() == 3 and (capped.weight == 3).any() and capped.info[0] > capped.weight.sum(), "the cap is hit"


def test_room_inside_points_and_vertices_lie_near_matter():
    """THE BOUND.  A point p with tsdf < 0 has an observation with sdf < 0: the pixel (px, py) it projects into holds a depth d with
    along - trunc <= d < along.  p's own image coordinates differ from the pixel centre's by at most half a pixel in u and in v, i.e. by
    at most sqrt(2) / (2 focal) in the normalised image plane, so the point r of the pixel's ray at p's distance lies within
    |q| sqrt(2) / (2 focal) of p (q = p - camera).  The surface point h the pixel saw is on that ray; in ray mode |r - h| = along - d <=
    trunc, so p is within trunc + |q| sqrt(2) / (2 focal) of h, which lies on an occupied voxel's box.  (In planar mode the same argument
    gives (zd - d) |cam| <= trunc |cam| along the ray; the bound asserted is the tighter one all the same, for both modes.)  A vertex
    lies on a tetrahedron edge one of whose ends is inside, at most sqrt(3) voxel from it."""
    vox = T.room()
    for mode in (T.PLANAR, T.RAY):
        vol, c2w = _room_volume(mode)
        pts = vol.points()
        cams = c2w[:4, :, 3]
        qmax = np.sqrt(((pts[..., None, :] - cams) ** 2).sum(-1)).max(axis=-1)               # the farthest of the cameras that can have seen it
        bound = 4 * S + qmax * np.sqrt(2.0) / (2 * T.FOCAL)
        inside = (vol.weight > 0) & (vol.tsdf < 0)
        dist = _box_distance(pts[inside], vox)
        print(f"room, mode {mode}: {int(inside.sum())} inside points, farthest from matter {dist.max():.3f} m, bound there >= {bound[inside].min():.3f} m")
        assert inside.sum() > 500 and (dist <= bound[inside]).all()
        values, _ = T.lattice(vol)
        mesh = _room_mesh(mode)
        vd = _box_distance(mesh["positions"].astype(np.float64), vox)
        print(f"room, mode {mode}: {len(vd)} vertices, farthest from matter {vd.max():.3f} m")
        assert (vd <= bound.max() + np.sqrt(3.0) * S).all()


@functools.lru_cache(maxsize=None)
def _room_mesh(mode):
    vol, _ = _room_volume(mode)
    values, _ = T.lattice(vol)
    return T.extract_observed(values, 0.0, T.ROOM_LO.astype(np.float32), np.full(3, S, np.float32))


def test_observed_only_extraction_rules():
    vol, _ = _room_volume(T.PLANAR)
    values, counts = T.lattice(vol)
    nan = np.isnan(values)
    assert counts.tolist() == [int((~nan).sum()), int(((vol.tsdf < 0) & ~nan).sum()), int((vol.best >= 0).sum())] and nan.any()
    mesh = _room_mesh(T.PLANAR)
    assert len(mesh["triangles"]) > 500
    for x, y, z, k in mesh["tets"]:
        for off in SF.tet_vertices(int(k)):
            assert not nan[x + off[0], y + off[1], z + off[2]], "a triangle's tetrahedron holds an unobserved corner"
    e = mesh["edges"]
    d = SF.DIRS[e[:, 3]]
    assert not nan[e[:, 0], e[:, 1], e[:, 2]].any() and not nan[e[:, 0] + d[:, 0], e[:, 1] + d[:, 1], e[:, 2] + d[:, 2]].any()
    used = np.zeros(len(mesh["positions"]), bool)
    used[mesh["triangles"].reshape(-1)] = True
    print(f"observed-only mesh: {len(used)} vertices, {int((~used).sum())} used by no triangle, {len(mesh['triangles'])} triangles")
    # the ordinary rule wraps the observed region in a shell: more of everything
    plain = SF.extract(values, 0.0, T.ROOM_LO.astype(np.float32), np.full(3, S, np.float32))
    assert len(plain["triangles"]) > len(mesh["triangles"])
    # without NaN the two rules are one
    for fill in (1.0, -1.0):
        filled = np.where(nan, np.float32(fill), values)
        a = SF.extract(filled, 0.0, T.ROOM_LO.astype(np.float32), np.full(3, S, np.float32))
        b = T.extract_observed(filled, 0.0, T.ROOM_LO.astype(np.float32), np.full(3, S, np.float32))
        for key in ("positions", "normals", "triangles"):
            assert a[key].tobytes() == b[key].tobytes(), (fill, key)


def test_vertex_attrs_against_a_vectorised_search():
    vol, _ = _room_volume(T.RAY)
    mesh = _room_mesh(T.RAY)
    rng = np.random.default_rng(3)
    extra = (T.ROOM_LO + rng.uniform(-0.1, 1.1, size=(200, 3)) * np.asarray(T.ROOM_SHAPE) * S).astype(np.float32)      # inside and outside the grid
    pos = np.concatenate([mesh["positions"], extra, np.array([[np.nan, 0, 0]], np.float32)])
    palette = rng.integers(0, 256, size=(29, 3)).astype(np.uint8)
    got = T.vertex_attrs(vol, pos, palette)
    with np.errstate(invalid="ignore"):
        cell = np.floor((pos.astype(np.float64) - T.ROOM_LO) / S)
    cell = np.clip(np.where(np.isnan(cell), 0, cell), 0, np.asarray(T.ROOM_SHAPE) - 1).astype(np.int64)
    NY, NZ = T.ROOM_SHAPE[1] + 1, T.ROOM_SHAPE[2] + 1
    lin0 = (cell[:, 0] * NY + cell[:, 1]) * NZ + cell[:, 2]
    offs = np.array([(dx * NY + dy) * NZ + dz for dx in (0, 1) for dy in (0, 1) for dz in (0, 1)])
    best = vol.best.reshape(-1)[lin0[:, None] + offs[None]].astype(np.float64)
    key = np.where(best >= 0, best, np.inf)
    pick = np.argmin(key, axis=1)                                              # the first minimum: the lowest lin
    word = vol.word.reshape(-1)[lin0 + offs[pick]]
    none = np.isinf(key.min(axis=1))
    label = np.where(none, -1, (word >> 24).astype(np.int64)).astype(np.int32)
    colour = np.where(none[:, None], 0, np.stack([word & 0xFF, (word >> 8) & 0xFF, (word >> 16) & 0xFF], axis=1)).astype(np.uint8)
    assert np.array_equal(got["label"], label) and np.array_equal(got["colour"], colour) and none.any() and (~none).sum() > 100
    assert np.array_equal(got["sem_colour"], np.where((label >= 0)[:, None], palette[np.maximum(label, 0)], 0).astype(np.uint8))


# ------------------------------------------------------------------ the library's boundary, without a GPU
def test_unit_is_built_bound_and_refuses_bad_arguments_before_any_hip_call():
    """The unit is in the build table without FMA contraction, its four symbols are bound, and an argument error returns MNF_ERR_INVALID
    on a machine with no GPU at all: the check comes before any HIP call (the pointers here are never dereferenced)."""
    import ctypes
    import importlib.util
    import os
    import apnrf_amd
    from apnrf_amd import _lib as L
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("_b", os.path.join(repo, "active-perception-using-neural-radiance-fields_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    assert "-ffp-contract=off" in b.SOURCES["tsdf.hip"]
    for name in ("mnf_tsdf_integrate", "mnf_tsdf_lattice", "mnf_tsdf_vertex_attrs", "mnf_surface_extract_observed"):
        assert name in L.SIGNATURES
    import __graft_entry__ as G
    G.build()
    lib = apnrf_amd.load_library()
    P, nan, inf = 0x10000, float("nan"), float("inf")
    c3 = lambda v: (ctypes.c_double * 3)(*v)
    good = dict(X=20, Y=9, Z=21, lo=c3([0, 0, 0]), voxel=0.05, trunc=0.2, mw=64, dmin=0.0, dmax=10.0, m=P, V=7, W=24, H=20, focal=12.0, d=P, dt=0, cs=4, kt=1, mode=0, info=P)

    def call(**bad):
        a = dict(good, **bad)
        return lib.mnf_tsdf_integrate(P, P, P, P, a["X"], a["Y"], a["Z"], a["lo"], a["voxel"], a["trunc"], a["mw"], a["dmin"], a["dmax"], a["m"], a["V"], a["W"], a["H"],
                                      a["focal"], a["d"], a["dt"], P, a["cs"], P, a["kt"], a["mode"], a["info"], None)

    for bad in (dict(X=0), dict(Y=1025), dict(lo=None), dict(lo=c3([nan, 0, 0])), dict(voxel=0.0), dict(voxel=inf), dict(trunc=0.0), dict(trunc=nan), dict(focal=-1.0),
                dict(focal=nan), dict(mw=0), dict(V=65536), dict(V=-1), dict(cs=2), dict(cs=5), dict(dt=2), dict(kt=2), dict(mode=2), dict(W=0), dict(dmin=-1.0), dict(dmax=inf),
                dict(m=None), dict(d=None), dict(info=None), dict(info=P + 4), dict(m=P + 4), dict(d=P + 2)):
        assert call(**bad) == -1, bad
        assert b"tsdf_integrate" in lib.mnf_last_error()
    assert call(V=0, m=None, d=None) == 0, "no views: MNF_OK, nothing launched"
    assert lib.mnf_tsdf_lattice(P, P, P, 20, 9, 21, 0, P, P, None) == -1 and lib.mnf_tsdf_lattice(P, P, P, 20, 9, 1025, 1, P, P, None) == -1
    assert lib.mnf_tsdf_vertex_attrs(P, P, 20, 9, 21, c3([0, 0, 0]), 0.05, P, -1, None, 0, P, P, None, None) == -1
    assert lib.mnf_tsdf_vertex_attrs(P, P, 20, 9, 21, c3([0, 0, 0]), 0.05, P, 4, None, 0, P, P, P, None) == -1, "sem_colour asks for a palette"
    f3 = (ctypes.c_float * 3)(1, 1, 1)
    assert lib.mnf_surface_extract_observed(P, 20, 9, 21, nan, f3, f3, 0, 0, None, None, None, P, P, 1 << 30, None) == -1
    assert lib.mnf_surface_extract_observed(P, 0, 9, 21, 0.0, f3, f3, 0, 0, None, None, None, P, P, 1 << 30, None) == -1
