"""The numpy restatement of the surface mesh (include/mi355nerf.h, "surface mesh"): marching tetrahedra on the Kuhn split over a scalar
lattice, the lattice points of an occupancy grid, the vertex attributes.  A plain loop over cells and tetrahedra; every float32 expression
is one numpy operation on float32 arrays, so each is rounded on its own, as the device unit (built without FMA contraction) evaluates it.
The orientation of the triangles is derived here from the rule, with float64 midpoints and numpy's cross product, not from the kernel's
table.  tests/test_surface_cpu.py holds this file to the definition; tests/test_gpu_surface.py holds the device to this file."""
import math

import numpy as np

DIRS = np.array([(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1)], np.int64)
TYPE_OF = {tuple(d): t for t, d in enumerate(DIRS.tolist())}
PERMS = [(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)]
F32 = np.float32


def tet_vertices(k):
    """The four vertices of tetrahedron k as offsets from the cell's lowest corner, int [4,3]."""
    e = np.eye(3, dtype=np.int64)
    p = PERMS[k]
    v1 = e[p[0]]
    return np.stack([np.zeros(3, np.int64), v1, v1 + e[p[1]], np.ones(3, np.int64)])


def case_triangles(k, s):
    """The triangles of tetrahedron k whose vertex i is inside iff bit i of s is set: a list of triangles, each three (i, j) pairs of
    tetrahedron vertices naming the edge of a crossing, oriented by the rule."""
    ins = [i for i in range(4) if (s >> i) & 1]
    outs = [i for i in range(4) if not (s >> i) & 1]
    if len(ins) in (0, 4):
        return []
    if len(ins) == 1:
        a, (b, c, d) = ins[0], outs
        tris = [[(a, b), (a, c), (a, d)]]
    elif len(ins) == 3:
        (a, b, c), d = ins, outs[0]
        tris = [[(a, d), (b, d), (c, d)]]
    else:
        (a, b), (c, d) = ins, outs
        tris = [[(a, c), (a, d), (b, d)], [(a, c), (b, d), (b, c)]]
    V = tet_vertices(k).astype(np.float64)
    w = V[outs].mean(axis=0) - V[ins].mean(axis=0)
    out = []
    for tri in tris:
        q = [0.5 * (V[i] + V[j]) for i, j in tri]
        dot = float(np.dot(np.cross(q[1] - q[0], q[2] - q[0]), w))
        assert dot != 0.0
        out.append(tri if dot > 0 else [tri[0], tri[2], tri[1]])
    return out


CASES = [[case_triangles(k, s) for s in range(16)] for k in range(6)]


def _finite(a):
    return np.isfinite(a)


def lattice_gradient(values):
    """[NX,NY,NZ,3] float32: central differences, one-sided on the boundary, a non-finite difference counting as 0."""
    v = np.asarray(values, F32)
    g = np.zeros(v.shape + (3,), F32)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(3):
            a = np.moveaxis(v, k, 0)
            d = np.empty_like(a)
            d[1:-1] = (a[2:] - a[:-2]) * F32(0.5)
            d[0] = a[1] - a[0]
            d[-1] = a[-1] - a[-2]
            d = np.where(_finite(d), d, F32(0))
            g[..., k] = np.moveaxis(d, 0, k)
    return g


def extract(values, iso, origin, step):
    """-> dict(positions [V,3] f32, normals [V,3] f32, triangles [T,3] int32, cases: the set of (k, s) met with 0 < s < 15)."""
    v = np.ascontiguousarray(values, F32)
    NX, NY, NZ = v.shape
    iso = F32(iso)
    origin = np.asarray(origin, F32).reshape(3)
    step = np.asarray(step, F32).reshape(3)
    with np.errstate(invalid="ignore"):
        inside = v > iso
    cross = np.zeros((NX, NY, NZ, 7), bool)
    for t, (dx, dy, dz) in enumerate(DIRS.tolist()):
        a = inside[:NX - dx, :NY - dy, :NZ - dz]
        b = inside[dx:, dy:, dz:]
        cross[:NX - dx, :NY - dy, :NZ - dz, t] = a != b
    vid = np.cumsum(cross.reshape(-1), dtype=np.int64).reshape(cross.shape) - 1
    vid[~cross] = -1
    px, py, pz, pt = np.nonzero(cross)                                # C order: ascending (lin(p), type)
    d = DIRS[pt]
    a = v[px, py, pz]
    b = v[px + d[:, 0], py + d[:, 1], pz + d[:, 2]]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        both = _finite(a) & _finite(b)
        t = np.where(both, (iso - a) / (b - a), F32(0.5)).astype(F32)
        P = np.stack([px, py, pz], axis=1).astype(F32)
        pos = (P + t[:, None] * d.astype(F32)) * step[None] + origin[None]
        G = lattice_gradient(v)
        ga = G[px, py, pz]
        gb = G[px + d[:, 0], py + d[:, 1], pz + d[:, 2]]
        g = ga + t[:, None] * (gb - ga)
        m = (-g) / step[None]
        length = np.sqrt((m[:, 0] * m[:, 0] + m[:, 1] * m[:, 1]) + m[:, 2] * m[:, 2])
        ok = (length > 0) & _finite(length)
        nrm = np.where(ok[:, None], m / np.where(ok, length, F32(1))[:, None], F32(0)).astype(F32)
    assert pos.dtype == F32 and nrm.dtype == F32
    tris, cases = [], set()
    tv = [tet_vertices(k) for k in range(6)]
    mixed = np.zeros((NX - 1, NY - 1, NZ - 1), bool)
    base = inside[:-1, :-1, :-1]
    for dx, dy, dz in DIRS.tolist():
        mixed |= inside[dx:NX - 1 + dx, dy:NY - 1 + dy, dz:NZ - 1 + dz] != base
    for x, y, z in np.argwhere(mixed).tolist():                      # C order: ascending cell; cells of one sign have no triangle
        c = np.array([x, y, z])
        for k in range(6):
            P4 = tv[k] + c
            s = sum(int(inside[tuple(P4[i])]) << i for i in range(4))
            if 0 < s < 15:
                cases.add((k, s))
            for tri in CASES[k][s]:
                idx = []
                for i, j in tri:
                    lo, hi = min(i, j), max(i, j)
                    p = P4[lo]
                    idx.append(int(vid[p[0], p[1], p[2], TYPE_OF[tuple((P4[hi] - p).tolist())]]))
                assert min(idx) >= 0
                tris.append(idx)
    return {"positions": pos, "normals": nrm, "triangles": np.asarray(tris, np.int32).reshape(-1, 3), "cases": cases}


def measure_terms(positions, triangles):
    """Per triangle, in float64: (area term, volume term)."""
    p = np.asarray(positions, np.float64)
    a, b, c = (p[np.asarray(triangles)[:, i]] for i in range(3))
    n = np.cross(b - a, c - a)
    area = 0.5 * np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
    bc = np.cross(b, c)
    vol = ((a[:, 0] * bc[:, 0] + a[:, 1] * bc[:, 1]) + a[:, 2] * bc[:, 2]) / 6.0
    return area, vol


def measure(positions, triangles):
    area, vol = measure_terms(positions, triangles)
    return math.fsum(area.tolist()), math.fsum(vol.tolist())


def directed_edges(triangles):
    t = np.asarray(triangles, np.int64)
    return np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])


def boundary_edges(triangles):
    """The directed edges whose reverse does not occur; raises if a directed edge occurs twice (the mesh is then not oriented)."""
    e = directed_edges(triangles)
    keys = e[:, 0] * (1 << 32) + e[:, 1]
    assert len(np.unique(keys)) == len(keys), "a directed edge occurs twice"
    rev = e[:, 1] * (1 << 32) + e[:, 0]
    return e[~np.isin(keys, rev)]


def euler_characteristic(n_vertices, triangles):
    e = directed_edges(triangles)
    und = np.unique(np.sort(e, axis=1), axis=0)
    return int(n_vertices) - len(und) + len(triangles)


# ------------------------------------------------------------------ lattice points
def lattice_points(binaries, refine, aabb):
    """-> (lin int32 [n], positions f32 [n,3], origin f32 [3], step f32 [3], lattice shape)."""
    b = np.asarray(binaries) != 0
    R = b.shape
    near = np.zeros(R, bool)
    for x, y, z in np.argwhere(b).tolist():
        near[max(x - 1, 0):x + 2, max(y - 1, 0):y + 2, max(z - 1, 0):z + 2] = True
    shape = tuple(r * refine + 1 for r in R)
    listed = np.zeros(shape, bool)
    for x, y, z in np.argwhere(near).tolist():                       # the points that touch cell (x, y, z)
        listed[x * refine:(x + 1) * refine + 1, y * refine:(y + 1) * refine + 1, z * refine:(z + 1) * refine + 1] = True
    aabb = np.asarray(aabb, F32).reshape(6)
    origin = aabb[:3].copy()
    step = ((aabb[3:] - aabb[:3]) / np.array([r * refine for r in R]).astype(F32)).astype(F32)
    ijk = np.argwhere(listed)
    lin = (ijk[:, 0] * shape[1] + ijk[:, 1]) * shape[2] + ijk[:, 2]
    pos = origin[None] + ijk.astype(F32) * step[None]
    assert pos.dtype == F32
    return lin.astype(np.int32), pos, origin, step, shape


# ------------------------------------------------------------------ vertex attributes
def vertex_attrs(rgb, sem, palette=None):
    rgb = np.asarray(rgb, F32)
    sem = np.asarray(sem, F32)
    with np.errstate(invalid="ignore"):
        u = np.minimum(np.maximum(np.where(np.isnan(rgb), F32(0), rgb), F32(0)), F32(1))
        colour = (u * F32(255.0) + F32(0.5)).astype(np.uint8)
        colour[np.isnan(rgb)] = 0
    label = np.full(sem.shape[0], -1, np.int32)
    for i, row in enumerate(sem):
        if np.isnan(row).any():
            continue
        best = 0
        for c in range(1, len(row)):
            if row[c] > row[best]:
                best = c
        label[i] = best
    out = {"colour": colour, "label": label}
    if palette is not None:
        pal = np.asarray(palette, np.uint8)
        out["sem_colour"] = np.where((label >= 0)[:, None], pal[np.maximum(label, 0)], np.uint8(0)).astype(np.uint8)
    return out


# ------------------------------------------------------------------ shapes the tests share
def ball(shape, radius, offset=0.13):
    """values = r - |p - c|, c = the lattice centre + offset per axis (lattice units)."""
    g = np.stack(np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij"), axis=-1)
    c = (np.array(shape, np.float64) - 1.0) / 2.0 + offset
    return (radius - np.linalg.norm(g - c, axis=-1)).astype(F32)


def torus(shape, R, r, offset=0.13):
    """values = r - distance to a circle of radius R in the plane x = centre."""
    g = np.stack(np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij"), axis=-1)
    c = (np.array(shape, np.float64) - 1.0) / 2.0 + offset
    p = g - c
    ring = np.sqrt(p[..., 1] ** 2 + p[..., 2] ** 2) - R
    return (r - np.sqrt(ring ** 2 + p[..., 0] ** 2)).astype(F32)


def single_point():
    v = np.zeros((5, 5, 5), F32)
    v[2, 2, 2] = 1.0
    return v
