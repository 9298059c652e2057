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


def integrate(vol, c2w, focal, depth, colour, classes, depth_mode=PLANAR):
    """Views in ascending order; depth [V,H,W] float32 or float16, colour [V,H,W,3 or 4] uint8, classes [V,H,W] uint8 or int64."""
    m = np.asarray(c2w, F64).reshape(-1, 3, 4)
    V, H, W = depth.shape
    assert m.shape[0] == V
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
