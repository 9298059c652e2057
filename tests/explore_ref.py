"""numpy restatement of the exploration map (csrc/explore.hip, include/mi355nerf.h "exploration map"): insert, counts, top-down view, frontier
cells with their multiplicities, frontier clusters and goals.  Written from the definition in the header: float32 for the walk, one rounding
per operation, the same selection rule; integers elsewhere; float64 for the goal distance.  Also the seeded inputs that the CPU and the GPU
tests share."""
import numpy as np

f32 = np.float32
MAX_INDEX = f32(2.0 ** 24)


def words_per_plane(res):
    n = int(res[0]) * int(res[1]) * int(res[2])
    return ((n + 31) // 32 + 1) & ~1


# ------------------------------------------------------------------ insert
def ray_setup(origins, viewdirs, depth, grid_min, voxel_size, max_range, acc=None, min_depth=0.0, min_acc=0.0):
    """Steps 1-4 of the definition -> dict(keep [N] bool, hit [N] bool, t [N] f32, a, b, n, s [N,3] int64, tm, td [N,3] f32); the rows of the
    arrays are meaningful where keep."""
    o, d = np.asarray(origins, f32).reshape(-1, 3), np.asarray(viewdirs, f32).reshape(-1, 3)
    dep = np.asarray(depth, f32).reshape(-1)
    vs, g = f32(voxel_size), np.asarray(grid_min, f32).reshape(1, 3)
    with np.errstate(all="ignore"):
        keep = ~np.isnan(dep) & ~(dep <= f32(min_depth))
        if acc is not None:
            keep &= ~(np.asarray(acc, f32).reshape(-1) < f32(min_acc))
        keep &= np.isfinite(o).all(axis=1) & np.isfinite(d).all(axis=1)
        hit = np.isfinite(dep) & (dep <= f32(max_range))
        t = np.where(hit, dep, f32(max_range)).astype(f32)
        inv = f32(1.0) / vs
        fa = np.floor((o - g) * inv)
        step = t[:, None] * d                                        # float32, rounded
        p = o + step                                                 # float32, rounded
        fb = np.floor((p - g) * inv)
        keep &= (np.abs(fa) < MAX_INDEX).all(axis=1) & (np.abs(fb) < MAX_INDEX).all(axis=1)      # a NaN fails
        a = np.where(keep[:, None], np.nan_to_num(fa, nan=0.0, posinf=0.0, neginf=0.0), 0).astype(np.int64)
        b = np.where(keep[:, None], np.nan_to_num(fb, nan=0.0, posinf=0.0, neginf=0.0), 0).astype(np.int64)
        n, s = np.abs(b - a), np.sign(b - a)
        edge = (a + (s > 0)).astype(f32) * vs
        tm = ((g + edge) - o) / d
        td = vs / np.abs(d)
    return dict(keep=keep, hit=hit, t=t, a=a, b=b, n=n, s=s, tm=tm.astype(f32), td=td.astype(f32))


def walk(setup, res=None, stop_outside=False):
    """Step 5 for all kept rays at once.  Yields (ray [M], voxel [M,3], last [M] bool) once per round: the voxel each still-walking ray stands
    in, and whether it is the ray's last.  A ray with n steps appears in n + 1 rounds.  With `stop_outside` (needs `res`) a ray is dropped once it
    has left the box for good, as the kernel does; the bits are the same."""
    act = np.nonzero(setup["keep"])[0]
    cur, n, s = setup["a"][act].copy(), setup["n"][act].copy(), setup["s"][act]
    tm, td = setup["tm"][act].copy(), setup["td"][act]
    rows = np.arange(3)[None]
    while act.size:
        if stop_outside:
            r = np.asarray(res, np.int64)[None]
            gone = (((s >= 0) & (cur >= r)) | ((s <= 0) & (cur < 0))).any(axis=1)
            if gone.any():
                act, cur, n, s, tm, td = act[~gone], cur[~gone], n[~gone], s[~gone], tm[~gone], td[~gone]
        last = n.sum(axis=1) == 0
        yield act, cur.copy(), last
        go = ~last
        act, cur, n, s, tm, td = act[go], cur[go], n[go], s[go], tm[go], td[go]
        if not act.size:
            break
        best = np.full(act.shape[0], -1)
        bt = np.zeros(act.shape[0], f32)
        for k in range(3):                                           # the first axis with steps left; a later one only with a strictly smaller tm
            with np.errstate(invalid="ignore"):
                take = (n[:, k] > 0) & ((best < 0) | (tm[:, k] < bt))
            best = np.where(take, k, best)
            bt = np.where(take, tm[:, k], bt)
        sel = rows == best[:, None]
        cur = cur + np.where(sel, s, 0)
        n = n - sel
        with np.errstate(all="ignore"):
            tm = np.where(sel, tm + td, tm).astype(f32)


def paths(setup):
    """-> {ray: [voxel, ...]} the complete walk of every kept ray (for the property tests)."""
    out = {int(i): [] for i in np.nonzero(setup["keep"])[0]}
    for ray, vox, _ in walk(setup):
        for i, v in zip(ray.tolist(), vox.tolist()):
            out[i].append(tuple(v))
    return out


def or_voxels(bits, plane, ijk, res):
    X, Y, Z = (int(r) for r in res)
    inside = ((ijk >= 0) & (ijk < np.array([X, Y, Z])[None])).all(axis=1)
    v = ijk[inside]
    lin = (v[:, 0] * Y + v[:, 1]) * Z + v[:, 2]
    np.bitwise_or.at(bits[plane], lin >> 5, np.uint32(1) << (lin & 31).astype(np.uint32))


def insert(bits, origins, viewdirs, depth, grid_min, voxel_size, res, max_range, acc=None, min_depth=0.0, min_acc=0.0, stats=None):
    """OR the pixels into bits uint32 [2, wpp] (step 6); -> bits.  `stats`, a list, gets the number of steps the kernel walks appended."""
    setup = ray_setup(origins, viewdirs, depth, grid_min, voxel_size, max_range, acc, min_depth, min_acc)
    steps = 0
    for ray, vox, last in walk(setup, res, stop_outside=True):
        occ = last & setup["hit"][ray]
        or_voxels(bits, 0, vox[~occ], res)
        or_voxels(bits, 1, vox[occ], res)
        steps += int((~last).sum())
    if stats is not None:
        stats.append(steps)
    return bits


def new_bits(res):
    return np.zeros((2, words_per_plane(res)), np.uint32)


def states_to_bits(state):
    """int8 [X,Y,Z] of -1 unknown / 0 free / 1 occupied / 2 occupied AND passed through -> uint32 [2, wpp]"""
    bits = new_bits(state.shape)
    or_voxels(bits, 0, np.argwhere((state == 0) | (state == 2)), state.shape)
    or_voxels(bits, 1, np.argwhere(state >= 1), state.shape)
    return bits


# ------------------------------------------------------------------ read-outs
def voxel_states(bits, res):
    """-> int8 [X,Y,Z]: 1 occupied, 0 free, -1 unknown; the tail bits are ignored."""
    n = int(res[0]) * int(res[1]) * int(res[2])
    b = ((bits[:, :, None] >> np.arange(32, dtype=np.uint32)[None, None]) & 1).astype(bool).reshape(2, -1)[:, :n]
    return np.where(b[1], 1, np.where(b[0], 0, -1)).astype(np.int8).reshape(res)


def counts(bits, res):
    st = voxel_states(bits, res)
    return np.array([(st == 0).sum(), (st == 1).sum(), (st == -1).sum()], np.int64)


def top_down(bits, res, y_lo=0, y_hi=None):
    st = voxel_states(bits, res)[:, y_lo:(res[1] if y_hi is None else y_hi), :]
    out = -np.ones((res[0], res[2]), np.int8)
    if st.shape[1]:
        out = np.where((st == 1).any(axis=1), 1, np.where((st == 0).any(axis=1), 0, -1)).astype(np.int8)
    return out


def frontiers(grid, max_frontiers=None):
    """-> (cells [F',2] i32 ascending row-major, mult [F'] i32, info [2] i64); F' = min(F, max_frontiers).  The multiplicity of a free cell is the
    number of columns x - 1, x, x + 1 inside the map that hold an unknown cell at z - 1, z or z + 1."""
    X, Z = grid.shape
    unknown = np.zeros((X + 2, Z + 2), bool)
    unknown[1:-1, 1:-1] = grid == -1
    column = unknown[:, :-2] | unknown[:, 1:-1] | unknown[:, 2:]     # [X+2, Z]: an unknown at z-1, z or z+1 of that (padded) column
    m = column[:-2].astype(np.int32) + column[1:-1] + column[2:]
    m = np.where(grid == 0, m, 0)
    cells = np.argwhere(m > 0).astype(np.int32)
    mult = m[m > 0].astype(np.int32)
    F = cells.shape[0]
    cap = F if max_frontiers is None else min(F, max_frontiers)
    return cells[:cap], mult[:cap], np.array([F, int(max_frontiers is not None and F > max_frontiers)], np.int64)


def frontier_clusters(cells, mult, current, eps2=1, min_samples=3, weighted=True, max_clusters=None):
    """-> dict(labels [F] i32, goals [K',2] i32, sizes [K'] i32, info [2] i64), K' = min(K, max_clusters)."""
    cells = np.asarray(cells, np.int64).reshape(-1, 2)
    F = cells.shape[0]
    w = np.asarray(mult, np.int64) if weighted else np.ones(F, np.int64)
    where = {(int(x), int(z)): i for i, (x, z) in enumerate(cells)}
    offs = [(dx, dz) for dx in range(-2, 3) for dz in range(-2, 3) if 0 < dx * dx + dz * dz <= eps2]
    nbrs = [[where[(int(x) + dx, int(z) + dz)] for dx, dz in offs if (int(x) + dx, int(z) + dz) in where] for x, z in cells]
    core = np.array([w[i] + sum(w[j] for j in nbrs[i]) >= min_samples for i in range(F)], bool)
    parent = np.arange(F)

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i

    for i in range(F):
        for j in nbrs[i]:
            if core[i] and core[j]:
                a, b = find(i), find(j)
                if a != b:
                    parent[max(a, b)] = min(a, b)
    roots = [i for i in range(F) if core[i] and find(i) == i]       # ascending: numbered by the smallest row-major core cell
    number = {r: k for k, r in enumerate(roots)}
    labels = -np.ones(F, np.int32)
    for i in range(F):
        if core[i]:
            labels[i] = number[find(i)]
        else:
            near = [number[find(j)] for j in nbrs[i] if core[j]]
            if near:
                labels[i] = min(near)
    K = len(roots)
    goals, sizes = np.zeros((K, 2), np.int32), np.zeros(K, np.int32)
    cx, cz = np.float64(current[0]), np.float64(current[1])
    for k in range(K):
        members = np.nonzero(labels == k)[0]
        dx, dz = cells[members, 0].astype(np.float64) - cx, cells[members, 1].astype(np.float64) - cz
        d2 = dx * dx + dz * dz
        goals[k] = cells[members[np.argmin(d2)]]                     # the first minimum: the lowest row-major cell
        sizes[k] = members.shape[0]
    cap = K if max_clusters is None else min(K, max_clusters)
    return dict(labels=labels, goals=goals[:cap], sizes=sizes[:cap], info=np.array([K, int(max_clusters is not None and K > max_clusters)], np.int64))


# ------------------------------------------------------------------ inputs shared by the CPU and the GPU tests
G_MIN, G_VS, MAX_RANGE = (0.5, 0.25, 1.0), 0.25, 2.5
MIN_DEPTH, MIN_ACC = 0.125, 0.375
RES_A, RES_B = (16, 8, 16), (7, 5, 9)


def seeded_rays(res, N, seed):
    """Rays with every edge the insert has, for a grid of `res` voxels of G_VS at G_MIN: origins inside and up to two voxels outside, end points
    inside and outside, and blocks of axis-parallel rays, rays that stay in one voxel, rays from voxel centres along exact diagonals (every tm
    ties), NaN / +-inf / 0 / negative depths, depths on and beyond max_range, non-finite origins and directions, acc on both sides of MIN_ACC."""
    rng = np.random.default_rng(seed)
    lo = np.array(G_MIN, f32)
    hi = lo + np.array(res, f32) * f32(G_VS)
    o = rng.uniform(lo - 0.5, hi + 0.5, (N, 3)).astype(f32)
    d = rng.normal(size=(N, 3)).astype(f32)
    d /= np.linalg.norm(d, axis=1, keepdims=True).astype(f32)
    depth = rng.uniform(0.0, 1.25 * MAX_RANGE, N).astype(f32)
    block = max(N // 16, 1)
    k = 0

    def take():
        nonlocal k
        sl = slice(k, min(k + block, N))
        k += block
        return sl

    sl = take()                                                      # axis-parallel, both signs
    m = sl.stop - sl.start
    d[sl] = 0.0
    d[np.arange(sl.start, sl.stop), rng.integers(0, 3, m)] = rng.choice([-1.0, 1.0], m).astype(f32)
    sl = take()                                                      # a == b: the ray ends in the voxel it starts in
    depth[sl] = rng.uniform(0.13, 0.2, sl.stop - sl.start).astype(f32) * f32(0.1) + f32(MIN_DEPTH)
    sl = take()                                                      # voxel centres, exact diagonals: tm ties at every corner
    m = sl.stop - sl.start
    cells = rng.integers(0, np.array(res), (m, 3))
    o[sl] = lo + (cells.astype(f32) + f32(0.5)) * f32(G_VS)
    signs = rng.choice([-1.0, 1.0], (m, 3)).astype(f32)
    signs[::3, 2] = 0.0                                              # some in a plane, some along one axis
    signs[1::5, 1] = 0.0
    d[sl] = signs
    depth[sl] = (rng.integers(1, 7, m).astype(f32) * f32(G_VS))      # t * d lands on voxel centres again
    sl = take()
    special = np.array([np.nan, np.inf, -np.inf, 0.0, -1.0, MIN_DEPTH, np.nextafter(f32(MIN_DEPTH), f32(1)), MAX_RANGE,
                        np.nextafter(f32(MAX_RANGE), f32(9)), 2 * MAX_RANGE, 1e30], f32)
    depth[sl] = special[np.arange(sl.stop - sl.start) % len(special)]
    sl = take()                                                      # non-finite origins and directions, huge ones (an index beyond 2^24)
    bad = np.array([np.nan, np.inf, -np.inf, 1e9, -1e9, 3e38], f32)
    idx = np.arange(sl.start, sl.stop)
    o[idx[::2], idx[::2] % 3] = bad[(idx[::2] // 2) % len(bad)]
    d[idx[1::2], idx[1::2] % 3] = bad[(idx[1::2] // 2) % len(bad)]
    acc = rng.uniform(0.0, 1.0, N).astype(f32)
    acc[::7] = MIN_ACC
    acc[3::7] = np.nextafter(f32(MIN_ACC), f32(0))
    acc[5::11] = np.nan
    return dict(o=o, d=d, depth=depth, acc=acc)


def ref_insert(case, res, sl=slice(None), bits=None, with_acc=True):
    if bits is None:
        bits = new_bits(res)
    return insert(bits, case["o"][sl], case["d"][sl], case["depth"][sl], G_MIN, G_VS, res, MAX_RANGE, acc=case["acc"][sl] if with_acc else None,
                  min_depth=MIN_DEPTH, min_acc=MIN_ACC if with_acc else 0.0)


def seeded_states(fill_free, fill_occ, seed, res=RES_A):
    """int8 [X,Y,Z] voxel states: a seeded mixture of free (0), occupied (1), both bits (2) and unknown (-1)."""
    u = np.random.default_rng(seed).random(res)
    st = -np.ones(res, np.int8)
    st[u < fill_free] = 0
    st[u > 1.0 - fill_occ] = 1
    st[(u > 1.0 - fill_occ / 2)] = 2
    return st


def room_states(res=RES_A):
    """A carved room with walls, an opening and an unseen remainder: long connected frontiers, a few separate ones."""
    X, Y, Z = res
    st = -np.ones(res, np.int8)
    st[2:X - 4, 1:Y - 1, 2:Z - 3] = 0
    st[2:X - 4, 1:Y - 1, 2] = 1                                      # a wall: no frontier along it
    st[2, 1:Y - 1, 2:Z - 3] = 1
    st[X - 2, 2, Z - 2] = 0                                          # an isolated free voxel: a frontier cell of multiplicity 3, never core at 3 unweighted
    st[0, 3, 0] = 0
    st[0, 3, 1] = 0
    return st


STATES = {"sparse": lambda: seeded_states(0.04, 0.02, 41), "dense": lambda: seeded_states(0.6, 0.2, 42), "room": room_states,
          "unknown": lambda: -np.ones(RES_A, np.int8), "free": lambda: np.zeros(RES_A, np.int8),
          "small": lambda: seeded_states(0.3, 0.1, 43, RES_B)}


# Two plus shapes, centres (2, 2) and (2, 4), that share the arm (2, 3).  At eps2 = 1, min_samples = 4, unit weights: the two centres (four
# neighbours each) are the only core cells and are not linked to each other, so they are clusters 0 and 1; (2, 3) has both as neighbours, is not
# core itself (1 + 2 < 4) and takes the smaller label; the other arms are border cells of one cluster each.
BORDER_CELLS = np.array([[1, 2], [1, 4], [2, 1], [2, 2], [2, 3], [2, 4], [2, 5], [3, 2], [3, 4]], np.int32)
BORDER_LABELS = [0, 1, 0, 0, 0, 1, 1, 0, 1]


def seeded_map2d(seed, shape=(12, 14), p=(0.35, 0.45, 0.2)):
    """A seeded -1 / 0 / 1 top-down map."""
    return np.random.default_rng(seed).choice(np.array([-1, 0, 1], np.int8), size=shape, p=p)
