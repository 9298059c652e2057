"""numpy restatement of the semantic object map (csrc/objmap.hip, include/mi355nerf.h "semantic object map"): insert, clusters, match.
Written from the definition in the header and from scripts/eval/eval_pipeline_offline.py:18-72, 110-142; float32 operations for the insert,
float64 for centroids and distances, the same expressions in the same order as the kernels, one rounding per operation."""
import numpy as np


def words_per_plane(res):
    n = int(res[0]) * int(res[1]) * int(res[2])
    return ((n + 31) // 32 + 1) & ~1


def first_argmax(sem):
    """First maximal logit per row, a NaN counting as the maximum (np.argmax)."""
    return np.argmax(sem, axis=-1).astype(np.int64)


def insert_voxels(origins, viewdirs, depth, grid_min, voxel_size, res, n_classes, first_class=1, sem=None, labels=None, acc=None,
                  min_depth=0.0, max_depth=np.inf, min_acc=0.0):
    """-> (keep [N] bool, cls [N] int64, ijk [N,3] int64) of the pixels; rows of ijk are valid where keep."""
    f32 = np.float32
    o, d = np.asarray(origins, f32).reshape(-1, 3), np.asarray(viewdirs, f32).reshape(-1, 3)
    dep = np.asarray(depth, f32).reshape(-1)
    cls = first_argmax(np.asarray(sem, f32).reshape(dep.shape[0], n_classes)) if sem is not None else np.asarray(labels).reshape(-1).astype(np.int64)
    keep = (cls >= first_class) & (cls < n_classes)
    with np.errstate(invalid="ignore", over="ignore"):
        keep &= np.isfinite(dep)
        keep &= ~(dep <= f32(min_depth)) & ~(dep > f32(max_depth))
        if acc is not None:
            keep &= ~(np.asarray(acc, f32).reshape(-1) < f32(min_acc))
        inv = f32(1.0) / f32(voxel_size)
        step = dep[:, None] * d                                      # float32, rounded
        p = o + step                                                 # float32, rounded
        rel = p - np.asarray(grid_min, f32)[None]
        f = np.floor(rel * inv)
        inside = (f >= f32(0.0)) & (f < np.asarray(res, f32)[None])
    keep &= inside.all(axis=1)
    ijk = np.where(keep[:, None], np.nan_to_num(f, nan=0.0, posinf=0.0, neginf=0.0), 0).astype(np.int64)
    return keep, cls, ijk


def pack_bits(cls, ijk, res, n_classes, bits=None):
    """OR voxels (cls [M], ijk [M,3]) into a uint32 [C, wpp] bit grid."""
    X, Y, Z = (int(r) for r in res)
    if bits is None:
        bits = np.zeros((n_classes, words_per_plane(res)), np.uint32)
    lin = (ijk[:, 0] * Y + ijk[:, 1]) * Z + ijk[:, 2]
    np.bitwise_or.at(bits, (cls, lin >> 5), (np.uint32(1) << (lin & 31).astype(np.uint32)))
    return bits


def insert(bits, origins, viewdirs, depth, grid_min, voxel_size, res, first_class=1, **kw):
    C = bits.shape[0]
    keep, cls, ijk = insert_voxels(origins, viewdirs, depth, grid_min, voxel_size, res, C, first_class, **kw)
    return pack_bits(cls[keep], ijk[keep], res, C, bits)


def grid_to_bits(occ):
    """bool [C,X,Y,Z] -> uint32 [C, wpp]"""
    C = occ.shape[0]
    c, x, y, z = np.nonzero(occ)
    return pack_bits(c, np.stack([x, y, z], 1), occ.shape[1:], C)


def set_voxels(bits, res):
    """-> (cls [M], lin [M]) of the set voxels, ordered by class and then by linear index; padding bits are ignored."""
    n = int(res[0]) * int(res[1]) * int(res[2])
    b = ((bits[:, :, None] >> np.arange(32, dtype=np.uint32)[None, None]) & 1).astype(bool).reshape(bits.shape[0], -1)[:, :n]
    cls, lin = np.nonzero(b)
    return cls.astype(np.int64), lin.astype(np.int64)


def counts(bits, res):
    cls, _ = set_voxels(bits, res)
    return np.bincount(cls, minlength=bits.shape[0]).astype(np.int64)


def unravel(lin, res):
    Y, Z = int(res[1]), int(res[2])
    return np.stack([lin // (Y * Z), (lin // Z) % Y, lin % Z], axis=1)


def _components(cls, ijk, res, link_r2):
    """Union-find over the set voxels: -> root [M] = the smallest rank of each voxel's component."""
    X, Y, Z = (int(r) for r in res)
    M = cls.shape[0]
    rank_of = {}
    for r in range(M):
        rank_of[(int(cls[r]), int(ijk[r, 0]), int(ijk[r, 1]), int(ijk[r, 2]))] = r
    parent = np.arange(M)

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i

    offs = [(dx, dy, dz) for dx in range(-2, 3) for dy in range(-2, 3) for dz in range(-2, 3)
            if 0 < dx * dx + dy * dy + dz * dz <= link_r2]
    for r in range(M):
        c, x, y, z = int(cls[r]), int(ijk[r, 0]), int(ijk[r, 1]), int(ijk[r, 2])
        for dx, dy, dz in offs:
            nx, ny, nz = x + dx, y + dy, z + dz
            if not (0 <= nx < X and 0 <= ny < Y and 0 <= nz < Z):
                continue
            j = rank_of.get((c, nx, ny, nz))
            if j is None:
                continue
            a, b = find(r), find(j)
            if a != b:
                parent[max(a, b)] = min(a, b)
    return np.array([find(i) for i in range(M)], dtype=np.int64)


def clusters(bits, res, grid_min, voxel_size, link_r2=4, min_cluster_voxels=1, max_voxels=None, max_clusters=None):
    """-> dict(rows [K',5] f64, cluster_counts [C] i64, info [4] i64, voxel_ids [M] i64, voxel_cluster [M] i32); K' = min(K, max_clusters).
    With more set voxels than max_voxels only `info` is meaningful (rows etc. are None)."""
    C = bits.shape[0]
    n = int(res[0]) * int(res[1]) * int(res[2])
    cls, lin = set_voxels(bits, res)
    M = cls.shape[0]
    if max_voxels is not None and M > max_voxels:
        return dict(rows=None, cluster_counts=None, info=np.array([M, 0, 1, 0], np.int64), voxel_ids=None, voxel_cluster=None)
    ijk = unravel(lin, res)
    root = _components(cls, ijk, res, link_r2)
    size = np.bincount(root, minlength=M) if M else np.zeros(0, np.int64)
    kept_root = np.nonzero((root == np.arange(M)) & (size >= min_cluster_voxels))[0].astype(np.int64)                    # ascending rank
    row_of_root = -np.ones(M, np.int64)
    row_of_root[kept_root] = np.arange(kept_root.shape[0])
    vc = row_of_root[root] if M else np.zeros(0, np.int64)
    K = kept_root.shape[0]
    rows = np.zeros((K, 5), np.float64)
    g64, v64 = np.asarray(grid_min, np.float32).astype(np.float64), np.float64(np.float32(voxel_size))
    sums = np.zeros((K, 3), np.int64)
    np.add.at(sums, vc[vc >= 0], ijk[vc >= 0])                       # int64: exact, whatever the order
    cnt = np.bincount(vc[vc >= 0], minlength=K).astype(np.float64)
    rows[:, 0], rows[:, 1] = cls[kept_root], cnt
    if K:
        rows[:, 2:] = g64[None] + (sums.astype(np.float64) / cnt[:, None] + 0.5) * v64     # one rounding per operation
    cc = np.bincount(cls[kept_root], minlength=C).astype(np.int64) if K else np.zeros(C, np.int64)
    cap = K if max_clusters is None else min(K, max_clusters)
    info = np.array([M, K, 0, int(max_clusters is not None and K > max_clusters)], np.int64)
    return dict(rows=rows[:cap], cluster_counts=cc, info=info, voxel_ids=cls * n + lin, voxel_cluster=vc.astype(np.int32))


def match(rows, n_classes, gt_locs, gt_class, det_dist_thresh=1.0):
    """eval_pipeline_offline.py:45-70 on cluster rows (class, count, cx, cy, cz) -> (detected [C] i32, match [K] i32, gt_match [G] i32)."""
    gt_locs = np.asarray(gt_locs, np.float64).reshape(-1, 3)
    gt_class = np.asarray(gt_class, np.int32).reshape(-1)
    K, G = rows.shape[0], gt_class.shape[0]
    detected = np.zeros(n_classes, np.int32)
    mt = -np.ones(K, np.int32)
    gm = -np.ones(G, np.int32)
    thresh = np.float64(det_dist_thresh)
    for k in range(K):
        c = int(rows[k, 0])
        best, arg = np.float64(10.0), -1
        for g in range(G):
            if gt_class[g] != c or gm[g] >= 0:
                continue
            dx, dy, dz = gt_locs[g, 0] - rows[k, 2], gt_locs[g, 1] - rows[k, 3], gt_locs[g, 2] - rows[k, 4]
            dist = np.sqrt((dx * dx + dy * dy) + dz * dz)
            if dist < thresh and dist < best:
                best, arg = dist, g
        if arg >= 0:
            gm[arg] = k
            mt[k] = arg
            detected[c] += 1
    return detected, mt, gm


# ------------------------------------------------------------------ inputs shared by the CPU and the GPU tests
RES = (16, 8, 16)


def seeded_grid(fill, seed, res=RES):
    return np.random.default_rng(seed).random(res) < fill


def snake_grid(res=RES, step=4):
    """A one-voxel-wide path through the whole grid: z-lines at every `step`-th (x, y), joined end to end; passes are `step` >= 3 apart, so
    for every link_r2 <= 8 the only links run along the path and the whole path is ONE component with the longest possible chains."""
    X, Y, Z = res
    occ = np.zeros(res, bool)
    top = False                                                      # which z end the path currently stands at
    ys = list(range(0, Y, step))
    for yi, y in enumerate(ys):
        xs = list(range(0, X, step))
        if yi % 2:
            xs.reverse()
        for xi, x in enumerate(xs):
            occ[x, y, :] = True
            top = not top
            zend = Z - 1 if top else 0
            if xi + 1 < len(xs):
                lo, hi = sorted((x, xs[xi + 1]))
                occ[lo:hi + 1, y, zend] = True
        if yi + 1 < len(ys):
            occ[xs[-1], y:ys[yi + 1] + 1, zend] = True
    return occ


GRIDS = {"fill8": lambda: seeded_grid(0.08, 280), "fill40": lambda: seeded_grid(0.40, 529), "snake": snake_grid, "full": lambda: np.ones(RES, bool)}


def _row(c, x, y, z, n=1):
    return [float(c), float(n), float(x), float(y), float(z)]


MATCH_CASES = {
    # a tie: objects 0 and 1 are both 0.5 from the cluster; the lowest index wins
    "tie": (np.array([_row(1, 0, 0, 0)]), [[0.5, 0, 0], [-0.5, 0, 0]], [1, 1], 1.0, [0, 1, 0], [0], [0, -1]),
    # a distance exactly equal to the threshold is rejected (strict <); just inside is taken
    "threshold": (np.array([_row(1, 0, 0, 0), _row(2, 0, 0, 0)]), [[1.0, 0, 0], [0.75, 0, 0]], [1, 2], 1.0, [0, 0, 1], [-1, 1], [-1, 1]),
    # one object, two clusters in reach: the first cluster in row order takes it, the second gets nothing
    "once": (np.array([_row(1, 0.5, 0, 0), _row(1, 0.25, 0, 0)]), [[0, 0, 0]], [1], 1.0, [0, 1, 0], [0, -1], [0]),
    # more clusters than objects; the nearest still-unmatched object is taken, not the nearest overall
    "more_clusters": (np.array([_row(1, 0, 0, 0), _row(1, 0.25, 0, 0), _row(1, 4, 0, 0)]), [[0.25, 0, 0], [0.75, 0, 0]], [1, 1], 1.0, [0, 2, 0],
                      [0, 1, -1], [0, 1]),
    # a class without objects, an object of a class without clusters, and a far object under a huge threshold: 10.0 still bounds it
    "empty_class": (np.array([_row(1, 0, 0, 0), _row(2, 0, 0, 0)]), [[0, 0, 0.5], [0, 0, 0], [0, 16, 0]], [2, 0, 1], 100.0, [0, 0, 1], [-1, 0], [1, -1, -1]),
    # 3-4-12 -> 13 is not below 10; 3-4-0 -> 5 is
    "pythagoras": (np.array([_row(1, 0, 0, 0)]), [[3, 4, 12], [3, 4, 0]], [1, 1], 100.0, [0, 1, 0], [1], [-1, 0]),
}
