"""The numpy restatement of TSDF fusion (include/mi355nerf.h, "TSDF fusion of captures"): the fusion operation by operation in the header's
order, every float64 expression one numpy operation so that each is rounded on its own, as the device unit (built without FMA
contraction) evaluates it; the lattice, the vertex attributes, and the observed-only extraction restated on top of surface_ref's
`tet_vertices` / `case_triangles`.  tests/test_tsdf_cpu.py holds this file to the definition; tests/test_gpu_tsdf.py holds the device to
this file."""
import numpy as np

import sensor_ref as SR
import surface_ref as SF

F32, F64 = np.float32, np.float64
PLANAR, RAY = 0, 1


class Volume:
    """The state over lattice points [X+1, Y+1, Z+1] of `cells` = (X, Y, Z) at `voxel` metres from `lo`."""

    def __init__(self, cells, lo, voxel, trunc, max_weight=64, min_depth=0.0, max_depth=10.0):
        self.cells = tuple(int(c) for c in cells)
        self.shape = tuple(c + 1 for c in self.cells)
        self.lo, self.voxel, self.trunc = np.asarray(lo, F64).reshape(3), F64(voxel), F64(trunc)
        self.max_weight, self.min_depth, self.max_depth = int(max_weight), F64(min_depth), F64(max_depth)
        self.tsdf = np.ones(self.shape, F32)
        self.weight = np.zeros(self.shape, np.int32)
        self.word = np.zeros(self.shape, np.uint32)
        self.best = np.full(self.shape, -1.0, F32)
        self.info = np.zeros(5, np.int64)

    def copy(self):
        v = Volume(self.cells, self.lo, self.voxel, self.trunc, self.max_weight, self.min_depth, self.max_depth)
        v.tsdf, v.weight, v.word, v.best, v.info = self.tsdf.copy(), self.weight.copy(), self.word.copy(), self.best.copy(), self.info.copy()
        return v

    def points(self):
        """w [NX, NY, NZ, 3] float64 = lo + (double)i * voxel."""
        ax = [self.lo[k] + np.arange(self.shape[k], dtype=F64) * self.voxel for k in range(3)]
        return np.stack(np.meshgrid(*ax, indexing="ij"), axis=-1)


def project(vol, m, W, H, focal, w=None):
    """Steps 1-4 of the header for one view m [3,4] and the points w [..., 3] (the lattice's own when None) -> (ok bool: zd > min_depth and
    the pixel lies in the image, px, py int64 (0 where not ok), zd, (q0, q1, q2))."""
    m = np.asarray(m, F64).reshape(3, 4)
    f = F64(focal)
    w = vol.points() if w is None else np.asarray(w, F64)
    with np.errstate(all="ignore"):
        R, c = m[:, :3], m[:, 3]
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
    return ok, px, py, zd, (q0, q1, q2)


def integrate(vol, c2w, focal, depth, colour, classes, depth_mode=PLANAR):
    """Views in ascending order; depth [V,H,W] float32 or float16, colour [V,H,W,3 or 4] uint8, classes [V,H,W] uint8 or int64."""
    m = np.asarray(c2w, F64).reshape(-1, 3, 4)
    V, H, W = depth.shape
    assert m.shape[0] == V
    w = vol.points()
    with np.errstate(all="ignore"):
        for v in range(V):
            ok, px, py, zd, (q0, q1, q2) = project(vol, m[v], W, H, focal, w)
            d = depth[v][py, px].astype(F64)
            invalid = ok & ~(np.isfinite(d) & (d > 0) & (d <= vol.max_depth))
            vol.info[2] += int(invalid.sum())
            ok &= ~invalid
            along = np.sqrt((q0 * q0 + q1 * q1) + q2 * q2) if depth_mode == RAY else zd
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


def lattice(vol, min_weight=1):
    """-> (values float32 [NX,NY,NZ]: -tsdf where weight >= min_weight else NaN, counts int64 [3])."""
    obs = vol.weight >= min_weight
    values = np.where(obs, -vol.tsdf, F32(np.nan)).astype(F32)
    return values, np.array([int(obs.sum()), int((obs & (vol.tsdf < 0)).sum()), int((vol.best >= 0).sum())], np.int64)


def vertex_attrs(vol, positions, palette=None):
    """A plain loop: the cell, its 8 corners in ascending lin, the smallest best >= 0 (the first on a tie)."""
    pos = np.asarray(positions, F32).reshape(-1, 3)
    n = pos.shape[0]
    colour, label = np.zeros((n, 3), np.uint8), np.full(n, -1, np.int32)
    with np.errstate(all="ignore"):
        cell = np.floor((pos.astype(F64) - vol.lo) / vol.voxel)
    for i in range(n):
        c = [0 if not cell[i, k] >= 0 else int(min(cell[i, k], vol.cells[k] - 1)) for k in range(3)]
        got = None
        for dx in (0, 1):
            for dy in (0, 1):
                for dz in (0, 1):
                    p = (c[0] + dx, c[1] + dy, c[2] + dz)
                    b = vol.best[p]
                    if b >= 0 and (got is None or b < got[0]):
                        got = (b, vol.word[p])
        if got is not None:
            wd = int(got[1])
            colour[i] = [wd & 0xFF, (wd >> 8) & 0xFF, (wd >> 16) & 0xFF]
            label[i] = wd >> 24
    out = {"colour": colour, "label": label}
    if palette is not None:
        pal = np.asarray(palette, np.uint8).reshape(-1, 3)
        ok = (label >= 0) & (label < pal.shape[0])
        out["sem_colour"] = np.where(ok[:, None], pal[np.where(ok, label, 0)], np.uint8(0)).astype(np.uint8)
    return out


def extract_observed(values, iso, origin, step):
    """surface_ref.extract with the one changed rule: a NaN point is unobserved; an edge carries a vertex only when its ends differ in
    inside-ness and neither is NaN; a tetrahedron emits only when none of its four vertices is NaN.  -> dict(positions, normals, triangles,
    tets: per triangle (x, y, z, k) of the tetrahedron that made it, edges: per vertex (x, y, z, type))."""
    v = np.ascontiguousarray(values, F32)
    NX, NY, NZ = v.shape
    iso = F32(iso)
    origin, step = np.asarray(origin, F32).reshape(3), np.asarray(step, F32).reshape(3)
    nan = np.isnan(v)
    with np.errstate(invalid="ignore"):
        inside = v > iso
    cross = np.zeros((NX, NY, NZ, 7), bool)
    for t, (dx, dy, dz) in enumerate(SF.DIRS.tolist()):
        sa, sb = np.s_[:NX - dx, :NY - dy, :NZ - dz], np.s_[dx:, dy:, dz:]
        cross[:NX - dx, :NY - dy, :NZ - dz, t] = (inside[sa] != inside[sb]) & ~nan[sa] & ~nan[sb]
    vid = np.cumsum(cross.reshape(-1), dtype=np.int64).reshape(cross.shape) - 1
    vid[~cross] = -1
    px, py, pz, pt = np.nonzero(cross)
    d = SF.DIRS[pt]
    a = v[px, py, pz]
    b = v[px + d[:, 0], py + d[:, 1], pz + d[:, 2]]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        both = np.isfinite(a) & np.isfinite(b)
        t = np.where(both, (iso - a) / (b - a), F32(0.5)).astype(F32)
        P = np.stack([px, py, pz], axis=1).astype(F32)
        pos = (P + t[:, None] * d.astype(F32)) * step[None] + origin[None]
        G = SF.lattice_gradient(v)
        ga = G[px, py, pz]
        gb = G[px + d[:, 0], py + d[:, 1], pz + d[:, 2]]
        g = ga + t[:, None] * (gb - ga)
        m = (-g) / step[None]
        length = np.sqrt((m[:, 0] * m[:, 0] + m[:, 1] * m[:, 1]) + m[:, 2] * m[:, 2])
        ok = (length > 0) & np.isfinite(length)
        nrm = np.where(ok[:, None], m / np.where(ok, length, F32(1))[:, None], F32(0)).astype(F32)
    assert pos.dtype == F32 and nrm.dtype == F32
    tris, tets = [], []
    tv = [SF.tet_vertices(k) for k in range(6)]
    for x in range(NX - 1):
        for y in range(NY - 1):
            for z in range(NZ - 1):
                cell_in = inside[x:x + 2, y:y + 2, z:z + 2]
                if cell_in.all() or not cell_in.any():
                    continue
                c = np.array([x, y, z])
                for k in range(6):
                    P4 = tv[k] + c
                    if any(nan[tuple(P4[i])] for i in range(4)):
                        continue
                    s = sum(int(inside[tuple(P4[i])]) << i for i in range(4))
                    for tri in SF.CASES[k][s]:
                        idx = []
                        for i, j in tri:
                            lo, hi = min(i, j), max(i, j)
                            p = P4[lo]
                            idx.append(int(vid[p[0], p[1], p[2], SF.TYPE_OF[tuple((P4[hi] - p).tolist())]]))
                        assert min(idx) >= 0
                        tris.append(idx)
                        tets.append((x, y, z, k))
    return {"positions": pos, "normals": nrm, "triangles": np.asarray(tris, np.int32).reshape(-1, 3), "tets": np.asarray(tets, np.int64).reshape(-1, 4),
            "edges": np.stack([px, py, pz, pt], axis=1)}


# ------------------------------------------------------------------ fixtures the tests share
S = 0.05
ROOM_SHAPE = (19, 9, 21)
ROOM_LO = np.array([-1.3, -0.2, 0.7])
W, H, FOCAL = 24, 20, 12.0


def room():
    """The (19, 9, 21) clutter grid at 0.05 m with all six boundary layers occupied and a pocket freed around the centre for the cameras."""
    v = SR.clutter_grid(ROOM_SHAPE, 0.03, 5).copy()
    rng = np.random.default_rng(17)
    X, Y, Z = ROOM_SHAPE
    shell = np.zeros(ROOM_SHAPE, bool)
    shell[0], shell[-1], shell[:, 0], shell[:, -1], shell[:, :, 0], shell[:, :, -1] = True, True, True, True, True, True
    col = rng.integers(0, 256, size=ROOM_SHAPE + (3,))
    cls = rng.integers(0, 29, size=ROOM_SHAPE)
    v = np.where(shell & ~SR.occupied(v), SR.pack(col[..., 0], col[..., 1], col[..., 2], cls), v).astype(np.uint32)
    cx, cy, cz = X // 2, Y // 2, Z // 2
    v[cx - 2:cx + 3, cy - 1:cy + 2, cz - 2:cz + 3] = np.uint32(0xFF000000)
    v.setflags(write=False)
    return v


def room_centre():
    return ROOM_LO + (np.asarray(ROOM_SHAPE) // 2 + 0.5) * S


def yaw_pose(position, degrees):
    a = np.deg2rad(degrees)
    c, s = np.cos(a), np.sin(a)
    R = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    return np.concatenate([R, np.asarray(position, F64).reshape(3, 1)], axis=1)


def room_poses(repeats=0):
    """Four views at the room centre turned 0, 90, 180 and -73 degrees about y, one looking away from 5 m outside (it misses the volume),
    then `repeats` repeats of the first."""
    c = room_centre()
    poses = [yaw_pose(c, a) for a in (0.0, 90.0, 180.0, -73.0)]
    poses.append(yaw_pose(c + np.array([0.0, 0.0, 5.0]), 180.0))           # looks along +z, away from the room behind it
    poses += [poses[0]] * repeats
    return np.stack(poses)


def room_captures(depth_mode, repeats=0):
    """-> (c2w [V,3,4], depth float32 [V,H,W], rgba uint8 [V,H,W,4], sem uint8 [V,H,W]) from sensor_ref.views, then planted pixels in view 1:
    NaN, inf, 0 and an over-range depth."""
    c2w = room_poses(repeats)
    out = SR.views(room(), ROOM_LO, S, c2w, W, H, FOCAL, 0.0, 100.0, ray_depth=depth_mode == RAY)
    depth = out["depth"].copy()
    depth[1, 3, 4], depth[1, 9, 12], depth[1, 10, 5], depth[1, 15, 20] = np.nan, np.inf, 0.0, 50.0
    return c2w, depth, out["rgba"], out["sem"]


# ------------------------------------------------------------------ general poses, long view lists and what a cull may assume of them
CELLS = (20, 9, 21)                                                          # the lattice the device tests fuse into: the room's, one cell wider in x
TRUNC = 4 * S
BLOCKS = ((4, 4, 16), (1, 4, 64), (2, 8, 16))                                # the shapes csrc/tsdf.hip can be built with; the first is the product's
MIN_ENTRY = 0.05


def volume(max_weight=64, min_depth=0.0, max_depth=10.0):
    return Volume(CELLS, ROOM_LO, S, TRUNC, max_weight=max_weight, min_depth=min_depth, max_depth=max_depth)


def general_pose(position, yaw, pitch, roll):
    """c2w [3,4] of Ry(yaw) Rx(pitch) Rz(roll), degrees: for generic angles none of the nine rotation entries is 0 or 1."""
    a, b, g = np.deg2rad([yaw, pitch, roll])
    Ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    Rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    Rz = np.array([[np.cos(g), -np.sin(g), 0], [np.sin(g), np.cos(g), 0], [0, 0, 1]])
    return np.concatenate([Ry @ Rx @ Rz, np.asarray(position, F64).reshape(3, 1)], axis=1)


def pose_pool(n, seed, spread=(0.3, 0.12, 0.35)):
    """n general poses around the room centre: any yaw, pitch and roll within 60 degrees, positions within `spread` metres of the centre per
    axis (the free pocket is 0.125 x 0.075 x 0.125 m, so most cameras sit among the clutter and see near hits).  A draw is repeated until
    every rotation entry has magnitude >= MIN_ENTRY: a naive draw leaves entries of 1e-4."""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        m = general_pose(room_centre() + rng.uniform(-1, 1, 3) * np.asarray(spread), rng.uniform(-180, 180), rng.uniform(-60, 60), rng.uniform(-60, 60))
        if np.abs(m[:, :3]).min() >= MIN_ENTRY:
            out.append(m)
    return np.stack(out)


def general_poses(n=24):
    return pose_pool(n, 29)


_GENERAL = {}


def general_captures(depth_mode):
    """-> (c2w [24,3,4], depth float32, rgba uint8, sem uint8) of `general_poses()` from sensor_ref.views, read-only."""
    if depth_mode not in _GENERAL:
        c2w = general_poses()
        out = SR.views(room(), ROOM_LO, S, c2w, W, H, FOCAL, 0.0, 100.0, ray_depth=depth_mode == RAY)
        got = (c2w, out["depth"], out["rgba"], out["sem"])
        for a in got:
            a.setflags(write=False)
        _GENERAL[depth_mode] = got
    return _GENERAL[depth_mode]


SKEW = np.array([[0.6, 0.3, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.9]])


def skewed(m):
    """The rotation block right-multiplied by SKEW: columns of norm 0.6, sqrt(1.09) and 1.9, the second sheared towards the first."""
    m = np.asarray(m, F64).reshape(-1, 3, 4).copy()
    m[:, :, :3] = m[:, :, :3] @ SKEW
    return m


def block_table(vol, block=BLOCKS[0]):
    """-> (index int64 [NX,NY,NZ] of the block each point lies in, z fastest as the kernel numbers its workgroups, blocks per axis)."""
    n = tuple(-(-vol.shape[k] // block[k]) for k in range(3))
    i = [np.arange(vol.shape[k]) // block[k] for k in range(3)]
    return (i[0][:, None, None] * n[1] + i[1][None, :, None]) * n[2] + i[2][None, None, :], n


def block_reach(vol, c2w, block=BLOCKS[0], counts=False):
    """bool [V, blocks]: some point of the block passes steps 3-4 for the view (with `counts`, how many do).  From `project` alone."""
    m = np.asarray(c2w, F64).reshape(-1, 3, 4)
    index, n = block_table(vol, block)
    w = vol.points()
    out = np.zeros((m.shape[0], int(np.prod(n))), np.int64)
    for v in range(m.shape[0]):
        out[v] = np.bincount(index[project(vol, m[v], W, H, FOCAL, w)[0]], minlength=out.shape[1])
    return out if counts else out > 0


def block_sphere(vol, block_index, block=BLOCKS[0]):
    """-> (centre [3], radius) of the smallest sphere about the box of the block's existing points."""
    index, n = block_table(vol, block)
    b = np.unravel_index(block_index, n)
    first = np.array([b[k] * block[k] for k in range(3)])
    last = np.minimum(first + np.asarray(block), np.asarray(vol.shape)) - 1
    return vol.lo + 0.5 * (first + last) * vol.voxel, 0.5 * float(vol.voxel) * float(np.linalg.norm(last - first))


def sphere_planes(vol, m, block_index, margin, block=BLOCKS[0], norms=None):
    """Plain float64 geometry, independent of `project`: is the block's bounding sphere, grown to (1 + margin) radius, wholly on the
    rejected side of (the near plane zd = min_depth, u = 0, u = W, v = 0, v = H)?  -> bool [5].

    In camera coordinates k = R^T q the admitted set of steps 3-4 is zd > min_depth with -zd W/2 <= xc focal < zd W/2 and the same for -yc
    and H: five half-spaces, each a linear form a . k >= b.  Over a ball of radius r in q the form R a . q varies by r |R a|, and
    |R a| <= sum |a_j| |column j of R| is the bound a cull can afford per view; `norms` replaces the three column norms (what a cull that
    assumed an orthonormal pose would use: (1, 1, 1))."""
    m = np.asarray(m, F64).reshape(3, 4)
    R = m[:, :3]
    centre, radius = block_sphere(vol, block_index, block)
    k = R.T @ (centre - m[:, 3])
    n = np.linalg.norm(R, axis=0) if norms is None else np.asarray(norms, F64)
    r = (1.0 + margin) * radius
    hw, hh, f = 0.5 * W, 0.5 * H, FOCAL
    forms = [(np.array([0.0, 0.0, -1.0]), float(vol.min_depth)),                 # zd >= min_depth
             (np.array([f, 0.0, -hw]), 0.0), (np.array([-f, 0.0, -hw]), 0.0),     # xc f + zd hw >= 0;  zd hw - xc f >= 0
             (np.array([0.0, -f, -hh]), 0.0), (np.array([0.0, f, -hh]), 0.0)]     # -yc f + zd hh >= 0;  zd hh + yc f >= 0
    return np.array([a @ k + r * (np.abs(a) @ n) < b for a, b in forms])


def sphere_clear(vol, m, block_index, margin, block=BLOCKS[0], norms=None):
    return bool(sphere_planes(vol, m, block_index, margin, block, norms).any())


B_NEVER, B_LATE, MARGIN = 1, 35, 0.1                                         # of the product's 36 blocks: two corners of the far z end, x and y apart
_VIEW_LISTS = {}


def view_list(V=600, depth_mode=PLANAR):
    """-> (c2w [V,3,4], depth float32 [V,H,W], rgba, sem): two full chunks of 256 views and a partial one, for the lattice of `volume()`.

    Poses come from a seeded pool of 3000 general poses.  Every view is `sphere_clear` of block B_NEVER at MARGIN, views 0 .. 255 of block
    B_LATE too, and the later ones are the pool's remaining ones in order (many reach B_LATE: tests/test_tsdf_cpu.py counts them).  The
    images are those of `general_captures`, view v taking capture v mod 24 with (1 + v mod 13) 2^-10 m added to every hit's depth: poses and
    images do not belong together, which the fusion cannot know.  Every ninth view from 330 on repeats the pose and the depth image of the
    view 70 before it, a view of another wave of the same chunk, under its own colours and classes: the two tie in |sdf|, and step 11's
    strict < gives the word to whichever comes first.  So no two views are interchangeable."""
    if (V, depth_mode) not in _VIEW_LISTS:
        pool, vol = pose_pool(3000, 31), volume()
        never = np.array([sphere_clear(vol, m, B_NEVER, MARGIN) for m in pool])
        late = np.array([sphere_clear(vol, m, B_LATE, MARGIN) for m in pool])
        head = np.nonzero(never & late)[0][:min(V, 256)]
        rest = np.setdiff1d(np.nonzero(never)[0], head)[:V - len(head)]
        c2w = pool[np.concatenate([head, rest])]
        assert c2w.shape[0] == V, "the pool is too small for this many views"
        _, depth, rgba, sem = general_captures(depth_mode)
        pick = np.arange(V) % depth.shape[0]
        offset = ((1 + np.arange(V) % 13) * 2.0 ** -10).astype(F32)
        depth = np.where(depth[pick] > 0, depth[pick] + offset[:, None, None], depth[pick]).astype(F32)
        for b in range(330, V, 9):
            c2w[b], depth[b] = c2w[b - 70], depth[b - 70]
        got = (c2w, depth, rgba[pick], sem[pick])
        for a in got:
            a.setflags(write=False)
        _VIEW_LISTS[(V, depth_mode)] = got
    return _VIEW_LISTS[(V, depth_mode)]
