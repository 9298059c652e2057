"""tests/tsdf_ref.py, the numpy restatement of TSDF fusion (include/mi355nerf.h "TSDF fusion of captures"), held to things it shares no code
with: the closed form of a wall seen head on, the geometry of a closed room (every point the volume calls inside lies near matter), the
rules of the observed-only extraction, and a vectorised search for the vertex attributes; under general rotations, to the sensor's own
pixel rays and to the closed form of a tilted plane.  The last group shows that the inputs of tests/test_gpu_tsdf.py discriminate: what
the 600-view list reaches in a kernel that culls views per block 256 at a time, that skewed poses need the column norms, that min_depth
binds.  No GPU."""
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


# ------------------------------------------------------------------ general poses: the restatement, and what the device tests' inputs reach
def _integrate_before_project(vol, c2w, focal, depth, colour, classes, depth_mode):
    """`tsdf_ref.integrate` as it stood before steps 1-4 moved into `tsdf_ref.project`, kept here word for word."""
    F32, F64 = np.float32, np.float64
    m = np.asarray(c2w, F64).reshape(-1, 3, 4)
    V, H, W = depth.shape
    f = F64(focal)
    w = vol.points()
    with np.errstate(all="ignore"):
        for v in range(V):
            R, c = m[v, :, :3], m[v, :, 3]
            q = w - c
            q0, q1, q2 = q[..., 0], q[..., 1], q[..., 2]
            xc = (q0 * R[0, 0] + q1 * R[1, 0]) + q2 * R[2, 0]
            yc = (q0 * R[0, 1] + q1 * R[1, 1]) + q2 * R[2, 1]
            zc = (q0 * R[0, 2] + q1 * R[1, 2]) + q2 * R[2, 2]
            zd = -zc
            ok = zd > vol.min_depth
            u = np.floor((xc / zd) * f + F64(W) * 0.5)
            vv = np.floor(((-yc) / zd) * f + F64(H) * 0.5)
            ok &= (u >= 0) & (u < W) & (vv >= 0) & (vv < H)
            px, py = np.where(ok, u, 0).astype(np.int64), np.where(ok, vv, 0).astype(np.int64)
            d = depth[v][py, px].astype(F64)
            invalid = ok & ~(np.isfinite(d) & (d > 0) & (d <= vol.max_depth))
            vol.info[2] += int(invalid.sum())
            ok &= ~invalid
            along = np.sqrt((q0 * q0 + q1 * q1) + q2 * q2) if depth_mode == T.RAY else zd
            sdf = d - along
            behind = ok & (sdf < -vol.trunc)
            vol.info[3] += int(behind.sum())
            ok &= ~behind
            s = np.minimum(1.0, sdf / vol.trunc)
            wt = vol.weight.astype(F64)
            new = ((vol.tsdf.astype(F64) * wt + s) / (wt + 1.0)).astype(F32)
            vol.tsdf = np.where(ok, new, vol.tsdf)
            vol.info[0] += int(ok.sum())
            vol.info[1] += int((ok & (vol.weight == 0)).sum())
            vol.weight = np.where(ok, np.minimum(vol.weight.astype(np.int64) + 1, vol.max_weight), vol.weight).astype(np.int32)
            a = np.abs(sdf)
            a32 = a.astype(F32)
            take = ok & (a <= vol.trunc) & ((vol.best < 0) | (a32 < vol.best))
            cls = classes[v][py, px].astype(np.int64)
            out = (cls < 0) | (cls > 255)
            vol.info[4] += int((take & out).sum())
            cls = np.where(out, 255, cls)
            col = colour[v][py, px]
            word = SR.pack(col[..., 0], col[..., 1], col[..., 2], cls)
            vol.best = np.where(take, a32, vol.best)
            vol.word = np.where(take, word, vol.word).astype(np.uint32)
    return vol


STATE = ("tsdf", "weight", "word", "best", "info")


def _same_state(a, b):
    return all(getattr(a, k).tobytes() == getattr(b, k).tobytes() for k in STATE)


def test_project_left_the_restatement_as_it_was():
    """Factoring steps 1-4 out changed no byte: the earlier body, kept above, run beside `integrate` on the room's captures (yaw poses,
    planted depths, an int64 class out of range, the cap) and on the general ones."""
    for mode in (T.PLANAR, T.RAY):
        c2w, depth, rgba, sem = T.room_captures(mode, repeats=2)
        sem64 = sem.astype(np.int64)
        sem64[0, 4:12, 6:18] = 300
        for args in ((c2w, T.FOCAL, depth, rgba, sem64), (c2w, T.FOCAL, depth.astype(np.float16), rgba[..., :3], sem)):
            a = T.integrate(T.volume(3), *args, mode)
            b = _integrate_before_project(T.volume(3), *args, mode)
            assert _same_state(a, b) and a.info[0] > 3000
        g = T.general_captures(mode)
        assert _same_state(T.integrate(T.volume(3), g[0], T.FOCAL, *g[1:], mode), _integrate_before_project(T.volume(3), g[0], T.FOCAL, *g[1:], mode))


def test_general_poses_are_general():
    c2w = T.general_poses()
    R = c2w[:, :, :3]
    assert c2w.shape == (24, 3, 4) and np.abs(R).min() >= T.MIN_ENTRY and np.abs(R).max() < 1
    assert np.abs(np.einsum("vij,vik->vjk", R, R) - np.eye(3)).max() < 1e-14 and (np.linalg.det(R) > 0).all()
    idx = np.floor((c2w[:, :, 3] - T.ROOM_LO) / S).astype(int)
    centre = np.asarray(T.ROOM_SHAPE) // 2
    outside = (np.abs(idx - centre) > np.array([2, 1, 2])).any(axis=1)
    depth = T.general_captures(T.PLANAR)[1]
    print(f"general poses: smallest rotation entry {np.abs(R).min():.4f}, {int(outside.sum())} of 24 cameras outside the free pocket, nearest hit "
          f"{depth[depth > 0].min():.4f} m, {int((depth.reshape(24, -1).min(axis=1) < T.TRUNC).sum())} views hold a hit nearer than trunc")
    assert outside.sum() >= 8 and (~outside).sum() >= 1 and (depth.reshape(24, -1).min(axis=1) < T.TRUNC).sum() >= 8
    K = T.skewed(c2w)[:, :, :3]
    n = np.linalg.norm(K, axis=1)
    assert np.allclose(n, [0.6, np.sqrt(1.09), 1.9]) and np.abs(np.einsum("vi,vi->v", K[:, :, 0], K[:, :, 1])).min() > 0.1, "norms on both sides of 1, and a shear"
    assert np.array_equal(T.skewed(c2w)[:, :, 3], c2w[:, :, 3])


def test_project_inverts_the_sensor_under_general_poses():
    """Points c + t dir(px, py) on the sensor's own pixel-centre rays (`sensor_ref.view_rays`) project into exactly (px, py): the ideal
    image coordinate is px + 0.5, half a pixel from either floor boundary, and the float64 chain moves it by some 1e-14."""
    c2w = T.general_poses()
    o, d, _, _ = SR.view_rays(c2w, T.W, T.H, T.FOCAL)
    vol = T.volume()
    py, px = np.meshgrid(np.arange(T.H), np.arange(T.W), indexing="ij")
    for v in range(len(c2w)):
        for t in (0.05, 0.37, 1.0, 7.5):
            ok, gx, gy, zd, _ = T.project(vol, c2w[v], T.W, T.H, T.FOCAL, o[v] + t * d[v])
            assert ok.all() and np.array_equal(gx, px) and np.array_equal(gy, py), (v, t)
            assert np.abs(zd - t).max() < 1e-13, "the camera's z component of dir is -1: planar depth is t"
            behind = T.project(vol, c2w[v], T.W, T.H, T.FOCAL, o[v] - t * d[v])[0]
            assert not behind.any()


def test_tilted_plane_matches_the_closed_form():
    """`test_wall_matches_the_closed_form` under general rotations.  A plane n . x = h tilted against the camera's axis by about 20
    degrees (n is the view direction plus 0.3 of the camera's x axis and 0.2 of its y axis), 0.35 m ahead; pixel (px, py) looks along
    dir = R k, k = (cam0, cam1, -1) from `sensor_ref.view_rays`, and meets the plane at t = (h - n . c) / (n . dir), which IS its planar
    depth (k_z = -1); its ray depth is t |k|.  The image is that, in float64, stored as float32.  One view is fused, and every observed
    point p holds tsdf = (float)min(1, (d(pixel(p)) - along(p)) / trunc), with pixel(p) and along(p) from k(p) = R^T (p - c) as a matrix
    product, which shares no expression with `project`.

    THE BOUND.  As for the wall.  t has a handful of float64 roundings (two dot products of three terms, a difference, a quotient, and
    |k| for ray depth) on numbers below 2, and along(p), the difference and the quotient by trunc a handful more: below 32 * 2^-53 * 2 m
    < 1e-14 m in all.  The depth is stored as float32: |d32 - d| <= 2^-24 d <= 2^-24 d_max.  The tsdf is stored as float32: 2^-24 |s|
    <= 2^-24.  So
        |tsdf - closed form| <= (2^-24 d_max + 1e-14) / trunc + 2^-24.
    A point whose image coordinate lies within 1e-9 of a pixel boundary may be assigned to either pixel by either chain and is left out
    (none is, with these poses); which points are observed is held too, away from the three thresholds by 1e-9."""
    vol0 = T.volume()
    pts = vol0.points()
    trunc = float(vol0.trunc)
    worst = {T.PLANAR: 0.0, T.RAY: 0.0}
    seen = inside = 0
    for m in T.general_poses()[:8]:
        R, c = m[:, :3], m[:, 3]
        n = R @ np.array([0.3, 0.2, -1.0])
        n /= np.linalg.norm(n)
        h = n @ (c + 0.35 * -R[:, 2])
        _, _, cam0, cam1 = SR.view_rays(m[None], T.W, T.H, T.FOCAL)
        k = np.stack([np.broadcast_to(cam0[None, :], (T.H, T.W)), np.broadcast_to(cam1[:, None], (T.H, T.W)), np.full((T.H, T.W), -1.0)], axis=-1)
        t = (h - n @ c) / (k @ R.T @ n)
        assert (t > 0).all() and t.max() < 2, "every pixel's ray meets the plane in front of the camera"
        kp = (pts - c) @ R                                                      # R^T (p - c), per point
        zd = -kp[..., 2]
        with np.errstate(all="ignore"):
            uf, vf = kp[..., 0] / zd * T.FOCAL + T.W / 2, -kp[..., 1] / zd * T.FOCAL + T.H / 2
        u, v = np.floor(uf), np.floor(vf)
        in_image = (zd > 0) & (u >= 0) & (u < T.W) & (v >= 0) & (v < T.H)
        edge = (np.abs(uf - np.round(uf)) < 1e-9) | (np.abs(vf - np.round(vf)) < 1e-9) | (np.abs(zd) < 1e-9)
        ui, vi = np.where(in_image, u, 0).astype(int), np.where(in_image, v, 0).astype(int)
        for mode in (T.PLANAR, T.RAY):
            d64 = t * np.linalg.norm(k, axis=-1) if mode == T.RAY else t
            depth = d64.astype(np.float32)[None]
            vol = T.integrate(T.volume(), m[None], T.FOCAL, depth, np.zeros((1, T.H, T.W, 3), np.uint8), np.zeros((1, T.H, T.W), np.uint8), mode)
            along = np.linalg.norm(pts - c, axis=-1) if mode == T.RAY else zd
            sdf = d64[vi, ui] - along
            want_obs = in_image & (sdf >= -trunc)
            sure = ~edge & (np.abs(sdf + trunc) > 1e-9)
            obs = vol.weight > 0
            assert (obs == want_obs)[sure].all() and int(edge.sum()) == 0
            sel = obs & sure
            err = np.abs(vol.tsdf.astype(np.float64) - np.minimum(1.0, sdf / trunc))[sel].max()
            bound = (2.0 ** -24 * d64.max() + 1e-14) / trunc + 2.0 ** -24
            print(f"tilted plane, mode {mode}: {int(sel.sum())} observed points, {int((vol.tsdf[sel] < 1).sum())} inside the truncation, tsdf error {err:.3e}, bound {bound:.3e}")
            assert sel.any() and (vol.tsdf[sel] < 0).any() and (vol.tsdf[sel] == 1).any(), "both sides of the plane and the clamp, for every pose"
            assert err <= bound
            worst[mode] = max(worst[mode], err)
            seen, inside = seen + int(sel.sum()), inside + int((vol.tsdf[sel] < 1).sum())
    print(f"tilted plane: {seen} observations over 8 poses and 2 modes, {inside} inside the truncation, worst error planar {worst[T.PLANAR]:.3e}, ray {worst[T.RAY]:.3e}")
    assert seen > 2000 and inside > 1000


def _reach_figures(reach):
    """Per chunk of 256 views: the most views that reach one block, the blocks reached from all four 64-view quarters, the blocks not reached."""
    out = []
    for lo in range(0, reach.shape[0], 256):
        chunk = reach[lo:lo + 256]
        quarters = np.stack([chunk[q:q + 64].any(axis=0) for q in range(0, 256, 64)])
        out.append((int(chunk.sum(axis=0).max()), int(quarters.all(axis=0).sum()), int((~chunk.any(axis=0)).sum())))
    return out


def test_view_list_reaches_every_branch_of_the_chunked_cull():
    """What the 600 views of `tsdf_ref.view_list` make a kernel do that takes views 256 at a time, a wave of 64 lanes testing 64 of them,
    for blocks of the product's 4 x 4 x 16 points; the same figures are printed for the two other shapes the unit can be built with."""
    c2w, depth, rgba, sem = T.view_list()
    assert c2w.shape[0] == 600 and np.abs(c2w[:, :, :3]).min() >= T.MIN_ENTRY
    vol = T.volume(3)
    for block in T.BLOCKS[1:]:
        print(f"blocks of {block}: (most survivors, blocks reached from all four quarters, blocks not reached) per chunk {_reach_figures(T.block_reach(vol, c2w, block))}")
    reach = T.block_reach(vol, c2w)
    figures = _reach_figures(reach)
    print(f"blocks of {T.BLOCKS[0]}: (most survivors, blocks reached from all four quarters, blocks not reached) per chunk {figures}")
    assert reach.shape == (600, 36)
    # (a) more than one wave's worth of survivors, from every wave
    chunk = reach[256:512]
    quarters = np.stack([chunk[q:q + 64].sum(axis=0) for q in range(0, 256, 64)])
    busy = (chunk.sum(axis=0) > 64) & (quarters > 0).all(axis=0)
    assert busy.any() and figures[0][0] > 64 and figures[1][0] > 64
    # (b) a block no view of the first chunk can reach, reached in the second and in the third
    late = [T.sphere_clear(vol, m, T.B_LATE, T.MARGIN) for m in c2w[:256]]
    n_late = [int(reach[lo:lo + 256, T.B_LATE].sum()) for lo in (0, 256, 512)]
    print(f"block {T.B_LATE}: clear of all {sum(late)} views of chunk 0 at margin {T.MARGIN}; reached by {n_late[1]} views of chunk 1 and {n_late[2]} of chunk 2")
    assert all(late) and n_late[0] == 0 and n_late[1] >= 1 and n_late[2] >= 1
    # (c) a block no view can reach, beside blocks that are written
    never = [T.sphere_clear(vol, m, T.B_NEVER, T.MARGIN) for m in c2w]
    neighbours = [T.B_NEVER - 1, T.B_NEVER + 2, T.B_NEVER + 6]                   # one block along z, y and x: 36 blocks are 6 x 3 x 2, z fastest
    print(f"block {T.B_NEVER}: clear of all {sum(never)} views at margin {T.MARGIN}; its neighbours {neighbours} are reached by {reach[:, neighbours].sum(axis=0).tolist()} views")
    assert all(never) and not reach[:, T.B_NEVER].any() and reach[:, neighbours].any(axis=0).all()
    # (d) order matters
    want = T.integrate(T.volume(3), c2w, T.FOCAL, depth, rgba, sem, T.PLANAR)
    back = T.integrate(T.volume(3), c2w[::-1], T.FOCAL, depth[::-1], rgba[::-1], sem[::-1], T.PLANAR)
    n_tsdf, n_word = int((want.tsdf.view(np.uint32) != back.tsdf.view(np.uint32)).sum()), int((want.word != back.word).sum())
    print(f"600 views reversed: {n_tsdf} tsdf values and {n_word} words differ; info {want.info.tolist()}, {int((want.weight == 3).sum())} points at the cap")
    assert n_tsdf > 100 and n_word > 20 and np.array_equal(want.weight, back.weight)
    # (e) every counter the images can move, and the cap
    assert want.info[0] > 0 and want.info[1] > 0 and want.info[3] > 0 and (want.weight == 3).any() and want.info[0] > want.weight.sum()
    index, _ = T.block_table(vol)
    assert (want.weight[index == T.B_NEVER] == 0).all() and (want.weight[index == T.B_LATE] > 0).any()
    # no two views are interchangeable
    assert len({(c2w[v].tobytes(), depth[v].tobytes(), rgba[v].tobytes()) for v in range(600)}) == 600 and len({depth[v].tobytes() for v in range(0, 312, 24)}) == 13


def test_skewed_poses_need_the_column_norms():
    """A cull that took the pose for orthonormal (norms 1, 1, 1) would drop (view, block) pairs that hold points steps 3-4 admit: for the
    skewed general poses `sphere_clear` with the norms forced to 1 rejects such pairs even at a margin of 0.1, and with the true norms it
    rejects none at margin 0.  The device test on these poses therefore fails for such a cull."""
    c2w = T.skewed(T.general_poses())
    vol = T.volume()
    n = T.block_reach(vol, c2w, counts=True)
    pairs = points = 0
    for v, b in zip(*np.nonzero(n)):
        assert not T.sphere_clear(vol, c2w[v], b, 0.0), "the bound with the true norms never rejects a reached pair"
        if T.sphere_clear(vol, c2w[v], b, T.MARGIN, norms=(1.0, 1.0, 1.0)):
            pairs, points = pairs + 1, points + int(n[v, b])
    print(f"skewed poses: {int((n > 0).sum())} reached (view, block) pairs; with the norms forced to 1 {pairs} of them, holding {points} points, are called clear")
    assert pairs > 0 and points > 0
    plain = T.general_poses()
    for v, b in zip(*np.nonzero(T.block_reach(vol, plain))):
        assert not T.sphere_clear(vol, plain[v], b, 0.0)


def test_min_depth_binds_on_the_general_captures():
    c2w, depth, rgba, sem = T.general_captures(T.PLANAR)
    near = T.integrate(T.volume(3, min_depth=0.4), c2w, T.FOCAL, depth, rgba, sem, T.PLANAR)
    zero = T.integrate(T.volume(3), c2w, T.FOCAL, depth, rgba, sem, T.PLANAR)
    assert 0 < near.info[0] < zero.info[0] and near.tsdf.tobytes() != zero.tsdf.tobytes() and near.word.tobytes() != zero.word.tobytes()
    only = [(v, b) for v in range(len(c2w)) for b in range(36)
            if T.sphere_planes(T.volume(min_depth=0.4), c2w[v], b, T.MARGIN)[0] and not T.sphere_clear(T.volume(), c2w[v], b, 0.0)]
    print(f"min_depth 0.4: {int(zero.info[0] - near.info[0])} observations fewer; {len(only)} (view, block) pairs are clear at the near plane only because of it")
    assert len(only) > 0
    reach = T.block_reach(T.volume(), c2w)
    assert any(reach[v, b] for v, b in only), "and some of those blocks hold points that min_depth = 0 admits"


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
