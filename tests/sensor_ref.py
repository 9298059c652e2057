"""The scene sensor in numpy (include/mi355nerf.h "scene sensor"): the walk, the view rays, the shading and the builders' host halves, each
float64 operation in the header's order (numpy rounds every one separately, as the unit built without FMA contraction does), plus the
brute-force slab intersection tests/test_sensor_cpu.py holds the walk to."""
import numpy as np

FREE = 0xFF
FACE_NEAR, FACE_NONE = 6, 255
SHADE = np.array([200, 200, 255, 150, 225, 225, 255], np.uint8)       # what apnrf_amd.sensor uses by default
BACKGROUND = 0xFF000000


def pack(r, g, b, cls):
    return (np.asarray(r, np.uint32) | (np.asarray(g, np.uint32) << 8) | (np.asarray(b, np.uint32) << 16) | (np.asarray(cls, np.uint32) << 24)).astype(np.uint32)


def occupied(voxels):
    return (voxels >> 24) != FREE


def bricks_words(shape):
    n = int(np.prod([(int(v) + 7) // 8 for v in shape]))
    return ((n + 31) // 32 + 1) & ~1


def build_bricks(voxels):
    """uint32 [words]: the brick mask of the header."""
    X, Y, Z = voxels.shape
    B = [(v + 7) // 8 for v in (X, Y, Z)]
    pad = np.zeros((B[0] * 8, B[1] * 8, B[2] * 8), bool)
    pad[:X, :Y, :Z] = occupied(voxels)
    any_ = pad.reshape(B[0], 8, B[1], 8, B[2], 8).any(axis=(1, 3, 5)).reshape(-1)
    words = np.zeros(bricks_words(voxels.shape), np.uint32)
    idx = np.nonzero(any_)[0]
    np.bitwise_or.at(words, idx >> 5, (np.uint32(1) << (idx & 31).astype(np.uint32)))
    return words


def walk(voxels, lo, s, origins, dirs, near, far):
    """-> (t_hit float64 [R] (-1 on a miss), hit int32 [R] (lin or -1), face uint8 [R] (255 on a miss), not_finite bool [R])."""
    X, Y, Z = voxels.shape
    N = np.array([X, Y, Z], np.int64)
    Nf = N.astype(np.float64)
    occ = occupied(voxels).reshape(-1)
    o, d = np.asarray(origins, np.float64).reshape(-1, 3), np.asarray(dirs, np.float64).reshape(-1, 3)
    R = o.shape[0]
    lo, s = np.asarray(lo, np.float64).reshape(3), np.float64(s)
    with np.errstate(all="ignore"):
        g = (o - lo) / s
        e = d / s
        finite = np.isfinite(o).all(1) & np.isfinite(d).all(1) & np.isfinite(g).all(1) & np.isfinite(e).all(1)
        step = np.where(e > 0, 1, np.where(e < 0, -1, 0)).astype(np.int64)
        inv = 1.0 / e
        alive = finite.copy()
        t_in = np.full(R, np.float64(near))
        t_out = np.full(R, np.float64(far))
        f_in = np.full(R, FACE_NEAR, np.int64)
        for a in range(3):
            moving = step[:, a] != 0
            t0 = (np.where(step[:, a] > 0, 0.0, Nf[a]) - g[:, a]) * inv[:, a]
            t1 = (np.where(step[:, a] > 0, Nf[a], 0.0) - g[:, a]) * inv[:, a]
            up = moving & (t0 > t_in)
            t_in = np.where(up, t0, t_in)
            f_in = np.where(up, 2 * a + (step[:, a] < 0), f_in)
            t_out = np.where(moving & (t1 < t_out), t1, t_out)
            alive &= moving | ((g[:, a] >= 0.0) & (g[:, a] < Nf[a]))
        alive &= t_in <= t_out
        p = np.floor(g + e * t_in[:, None])
        c = np.where(p < 0.0, 0.0, np.where(p > Nf - 1, Nf - 1, p))
        c = np.where(np.isfinite(c), c, 0.0).astype(np.int64)
        pos = (step > 0).astype(np.int64)
        f = np.where(step != 0, ((c + pos).astype(np.float64) - g) * inv, np.inf)
        t = t_in.copy()
        face = f_in.copy()
        t_hit = np.full(R, -1.0)
        hit = np.full(R, -1, np.int64)
        out_face = np.full(R, FACE_NONE, np.int64)
        rows = np.arange(R)
        for _ in range(int(N.sum()) + 2):
            if not alive.any():
                break
            lin = (c[:, 0] * Y + c[:, 1]) * Z + c[:, 2]
            h = alive & occ[lin]
            t_hit = np.where(h, np.maximum(t, t_in), t_hit)
            hit = np.where(h, lin, hit)
            out_face = np.where(h, face, out_face)
            alive &= ~h
            a = np.zeros(R, np.int64)
            a = np.where(f[:, 1] < f[rows, a], 1, a)
            a = np.where(f[:, 2] < f[rows, a], 2, a)
            fa = f[rows, a]
            alive &= fa <= t_out
            sa = step[rows, a]
            ca = c[rows, a] + sa
            alive &= (ca >= 0) & (ca < N[a])
            fn = ((ca + (sa > 0)).astype(np.float64) - g[rows, a]) * inv[rows, a]
            c[rows[alive], a[alive]] = ca[alive]
            f[rows[alive], a[alive]] = fn[alive]
            t = np.where(alive, fa, t)
            face = np.where(alive, 2 * a + (sa < 0), face)
        assert not alive.any(), "a walk did not end within X + Y + Z steps"
    return t_hit, hit.astype(np.int32), out_face.astype(np.uint8), ~finite


def view_rays(c2w, W, H, focal):
    """-> (origins [V,H,W,3], dirs [V,H,W,3], cam0 [W], cam1 [H]) in float64, the header's order."""
    m = np.asarray(c2w, np.float64).reshape(-1, 3, 4)
    f = np.float64(focal)
    cam0 = ((np.arange(W, dtype=np.float64) - np.float64(W) * 0.5) + 0.5) / f
    cam1 = ((np.arange(H, dtype=np.float64) - np.float64(H) * 0.5) + 0.5) / f * -1.0
    c0, c1 = cam0[None, None, :, None], cam1[None, :, None, None]
    with np.errstate(all="ignore"):
        d = (c0 * m[:, None, None, :, 0] + c1 * m[:, None, None, :, 1]) + -1.0 * m[:, None, None, :, 2]
    o = np.broadcast_to(m[:, None, None, :, 3], d.shape)
    return o, d, cam0, cam1


def views(voxels, lo, s, c2w, W, H, focal, near, far, ray_depth=False, shade=SHADE, background=BACKGROUND):
    """-> dict(rgba uint8 [V,H,W,4], depth float32 [V,H,W], depth64 (before the cast), sem uint8, hit int32, face uint8, info int64 [2])."""
    o, d, cam0, cam1 = view_rays(c2w, W, H, focal)
    V = o.shape[0]
    t, hit, face, bad = walk(voxels, lo, s, o.reshape(-1, 3), d.reshape(-1, 3), near, far)
    got = hit >= 0
    word = voxels.reshape(-1)[np.where(got, hit, 0)].astype(np.uint32)
    k = np.asarray(shade, np.uint32)[np.where(got, face, 0)]
    ch = [(((word >> sh) & 0xFF) * k + 127) // 255 for sh in (0, 8, 16)]
    px = np.where(got, ch[0] | (ch[1] << 8) | (ch[2] << 16) | np.uint32(0xFF000000), np.uint32(background)).astype("<u4")
    rgba = px.view(np.uint8).reshape(V, H, W, 4)
    scale = np.sqrt((cam0[None, :] * cam0[None, :] + cam1[:, None] * cam1[:, None]) + 1.0)
    t3 = t.reshape(V, H, W)
    d64 = np.where(got.reshape(V, H, W), t3 * scale[None] if ray_depth else t3, 0.0)
    sem = np.where(got, word >> 24, 0).astype(np.uint8).reshape(V, H, W)
    info = np.array([int((~got).sum()), int(bad.sum())], np.int64)
    return {"rgba": rgba, "depth": d64.astype(np.float32), "depth64": d64, "sem": sem, "hit": hit.reshape(V, H, W), "face": face.reshape(V, H, W), "info": info}


# ------------------------------------------------------------------ brute force
def brute(voxels, lo, s, origins, dirs, near, far):
    """Slab intersection of every ray with every occupied voxel, in grid coordinates, no walk: voxel i spans [i, i + 1] along an axis and
    the ray is between its two faces for t from en = (i - g) / e to ex = (i + 1 - g) / e (swapped for e < 0; one division each; an axis
    with e = 0 is inside for every t where i <= g < i + 1).

    Ties follow the definition by symbolic perturbation, not by re-running it: an event is the pair (time, axis), ordered by time and
    then by axis, which is "the lowest axis crosses first"; the ray starts at START = (t_in, -1), t_in = the larger of `near` and the
    box's entry times, in the cell floor() puts it in.  So a crossing INTO a slab at exactly t_in has already happened for an axis moving
    up (floor) and for the grid's last slab of an axis moving down (the clamp): its event is START; a slab LEFT at exactly t_in by an axis
    moving up was never entered, unless it is the grid's last (the clamp again).  A voxel is met iff every entry event precedes every exit event and the latest entry is not beyond
    `far`; its time is that of the latest entry event.  -> (t float64 [R] (-1: miss), lin int64 [R], gap float64 [R]: the entry time of the
    runner-up voxel minus t, inf where there is none)."""
    N = np.asarray(voxels.shape, np.float64)
    idx = np.argwhere(occupied(voxels)).astype(np.float64)
    lins = np.nonzero(occupied(voxels).reshape(-1))[0]
    o, d = np.asarray(origins, np.float64).reshape(-1, 3), np.asarray(dirs, np.float64).reshape(-1, 3)
    lo = np.asarray(lo, np.float64)
    g, e = (o - lo) / s, d / s
    R, M = o.shape[0], idx.shape[0]
    t_res, lin_res, gap = np.full(R, -1.0), np.full(R, -1, np.int64), np.full(R, np.inf)
    if M == 0:
        return t_res, lin_res, gap
    later = lambda t1, r1, t2, r2: (t1 > t2) | ((t1 == t2) & (r1 > r2))
    with np.errstate(all="ignore"):
        for r in range(R):
            t_in = np.float64(near)
            for a in range(3):
                if e[r, a] != 0.0:
                    t_in = max(t_in, min((0.0 - g[r, a]) / e[r, a], (N[a] - g[r, a]) / e[r, a]))
            ok = np.ones(M, bool)
            Et, Er = np.full(M, t_in), np.full(M, -1.0)                                # the latest entry event so far
            Xt, Xr = np.full(M, np.inf), np.full(M, 9.0)                               # the earliest exit event so far
            for a in range(3):
                if e[r, a] == 0.0:
                    ok &= (idx[:, a] <= g[r, a]) & (g[r, a] < idx[:, a] + 1.0)
                    continue
                ta, tb = (idx[:, a] - g[r, a]) / e[r, a], ((idx[:, a] + 1.0) - g[r, a]) / e[r, a]
                up = e[r, a] > 0.0
                en, ex = (ta, tb) if up else (tb, ta)
                at_start = (en < t_in) | ((en == t_in) & (up | (idx[:, a] == N[a] - 1)))
                et, er = np.where(at_start, t_in, en), np.where(at_start, -1.0, float(a))
                ok &= ((ex > t_in) | ((ex == t_in) & (idx[:, a] == N[a] - 1))) if up else (ex >= t_in)
                swap = later(et, er, Et, Er)
                Et, Er = np.where(swap, et, Et), np.where(swap, er, Er)
                swap = later(Xt, Xr, ex, float(a))
                Xt, Xr = np.where(swap, ex, Xt), np.where(swap, float(a), Xr)
            ok &= later(Xt, Xr, Et, Er) & (Et <= far)
            if not ok.any():
                continue
            cand = np.nonzero(ok)[0]
            order = np.lexsort((Er[cand], Et[cand]))
            first = cand[order[0]]
            t_res[r], lin_res[r] = Et[first], lins[first]
            if len(order) > 1:
                gap[r] = Et[cand[order[1]]] - Et[first]
    return t_res, lin_res, gap


# ------------------------------------------------------------------ fixtures
def clutter_grid(shape=(19, 9, 21), p=0.03, seed=5, floor=True):
    rng = np.random.default_rng(seed)
    X, Y, Z = shape
    occ = rng.uniform(size=shape) < p
    if floor:
        occ[:, 0, :] = True
    cls = rng.integers(0, 29, size=shape)
    col = rng.integers(0, 256, size=shape + (3,))
    return np.where(occ, pack(col[..., 0], col[..., 1], col[..., 2], cls), np.uint32(0xFF000000)).astype(np.uint32)


def ray_mix(shape, lo, s, n=3000, seed=11):
    """Origins inside and outside the grid, directions towards it and away; every tenth ray has one direction component exactly 0."""
    rng = np.random.default_rng(seed)
    ext = np.asarray(shape, np.float64) * s
    lo = np.asarray(lo, np.float64)
    inside = lo + rng.uniform(0.02, 0.98, size=(n, 3)) * ext
    outside = lo + rng.uniform(-0.6, 1.6, size=(n, 3)) * ext
    o = np.where((np.arange(n) % 2 == 0)[:, None], inside, outside)
    target = lo + rng.uniform(0.0, 1.0, size=(n, 3)) * ext
    d = (target - o) * rng.uniform(0.2, 3.0, size=(n, 1))
    d[::10, rng.integers(0, 3)] = 0.0
    d[5::10, :] = rng.normal(size=(len(d[5::10]), 3))
    return o, d


def lattice_rays(shape, lo, s):
    """Rays through lattice corners: integer g and integer slope ratios, so that two or three crossing times tie again and again."""
    lo = np.asarray(lo, np.float64)
    o, d = [], []
    for start in ((0, 0, 0), (2, 1, 3), (1, 4, 1), (shape[0], shape[1], shape[2]), (shape[0], 0, shape[2]), (3, shape[1], 0)):
        for slope in ((1, 1, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (2, 1, 1), (1, 2, 1), (2, 1, 2), (1, 1, 2), (3, 1, 0), (1, 0, 0), (0, 0, 1)):
            for sign in ((1, 1, 1), (-1, 1, 1), (1, -1, -1), (-1, -1, -1), (1, 1, -1)):
                o.append(lo + np.asarray(start, np.float64) * s)
                d.append(np.asarray(slope, np.float64) * np.asarray(sign, np.float64) * s)
    return np.array(o), np.array(d)


# ------------------------------------------------------------------ builders
def cell_hash(cx, cy, cz, num_classes=29):
    """standin.analytic_targets' class of a 0.2 m cell (standin.py:56-57), int64."""
    cx, cy, cz = (np.asarray(v, np.int64) for v in (cx, cy, cz))
    return ((cx * 73856093) ^ (cy * 19349663) ^ (cz * 83492791)) % num_classes


def first_point_wins(points, lo, s, shape):
    """-> (lin of every occupied voxel, ascending; the index of the lowest point in each), by a plain loop."""
    seen = {}
    for i, p in enumerate(np.asarray(points, np.float64)):
        c = np.floor((p - lo) / s).astype(np.int64)
        lin = int((c[0] * shape[1] + c[1]) * shape[2] + c[2])
        seen.setdefault(lin, i)
    keys = sorted(seen)
    return np.array(keys, np.int64), np.array([seen[k] for k in keys], np.int64)
