"""The scene sensor's definition, held to brute force on the host (no GPU): the numpy restatement of the walk (tests/sensor_ref.py, which
tests/test_gpu_sensor.py compares the kernels with byte for byte) against the slab intersection of every ray with every occupied voxel,
and the host halves of the scene builders.

THE BOUND on t.  Both sides start from the same g = (o - lo) / s and e = d / s.  The walk's time of a face at integer i is
((i - g) * (1 / e)): the difference (one rounding, the same double on both sides), the reciprocal (one rounding) and the product (one
rounding).  Brute force forms (i - g) / e: the same difference and one rounding.  With u = 2^-53 the walk's value is x (1 + d1)(1 + d2)
and brute force's x (1 + d3), |d| <= u, x the exact quotient of the rounded difference: they differ by at most (3 u + 3 u^2 + u^3) |x| <
3 u (1 + 2 u) |t| for either computed t.  max(., near), max(t, t_in) and the comparisons add no rounding.  So
    |t_walk - t_brute| <= BOUND * max(|t_walk|, |t_brute|),  BOUND = 3 * 2^-53 * (1 + 2^-51),
which is 1.5 float64 epsilons: at most 3 ulp and usually 1.  Hit or miss must agree on every ray.  The first voxel may differ only where
brute force's two earliest entry times lie within that bound of each other; the fixtures need no such excuse and the tests say so."""
import numpy as np
import pytest

import sensor_ref as SR

BOUND = 3 * 2.0 ** -53 * (1 + 2.0 ** -51)
SHAPE, LO, S = (19, 9, 21), np.array([-1.3, -0.2, 0.7]), 0.05
NEAR, FAR = 0.0, 100.0
_CACHE = {}


def scene():
    if "scene" not in _CACHE:
        v = SR.clutter_grid(SHAPE, 0.03, 5)
        v.setflags(write=False)
        _CACHE["scene"] = v
    return _CACHE["scene"]


def compare(name, o, d, near=NEAR, far=FAR, voxels=None):
    """The restatement against brute force on one ray set -> the number of hits."""
    v = scene() if voxels is None else voxels
    t, hit, face, bad = SR.walk(v, LO, S, o, d, near, far)
    bt, blin, gap = SR.brute(v, LO, S, o, d, near, far)
    assert not bad.any()
    got, want = hit >= 0, blin >= 0
    assert np.array_equal(got, want), f"{name}: hit/miss differs on rays {np.nonzero(got != want)[0][:8].tolist()}"
    err = np.abs(t - bt)[got]
    lim = BOUND * np.maximum(np.abs(t), np.abs(bt))[got]
    print(f"{name}: {int(got.sum())} hits of {len(t)} rays, largest |dt| / bound {np.max(err / np.maximum(lim, 1e-300), initial=0.0):.3f}")
    assert (err <= lim).all(), f"{name}: t differs by up to {err.max():.3e}"
    other = got & (hit != blin)
    assert not other.any(), f"{name}: another first voxel on rays {np.nonzero(other)[0][:8].tolist()} (gaps {gap[other][:8].tolist()})"
    assert (face[got] <= 6).all() and (face[~got] == SR.FACE_NONE).all() and (t[~got] == -1.0).all()
    return int(got.sum())


def test_walk_equals_brute_force_on_the_ray_mix():
    o, d = SR.ray_mix(SHAPE, LO, S)
    assert (d[::10] == 0.0).any(axis=1).all()
    assert compare("mix", o, d) > 500


def test_walk_through_lattice_corners():
    """Integer g and integer slope ratios (a voxel edge of 2^-4 keeps both exact): crossing times tie exactly, two and three at a time,
    from the first step on, and the lowest axis goes first."""
    s = 0.0625
    lo = np.array([-2.0, 1.0, 3.0]) * s
    o, d = SR.lattice_rays(SHAPE, lo, s)
    assert np.array_equal((o - lo) / s, np.rint((o - lo) / s)) and np.array_equal(d / s, np.rint(d / s))
    v = scene()
    t, hit, face, bad = SR.walk(v, lo, s, o, d, NEAR, FAR)
    bt, blin, gap = SR.brute(v, lo, s, o, d, NEAR, FAR)
    got = hit >= 0
    assert np.array_equal(got, blin >= 0), f"hit/miss differs on rays {np.nonzero(got != (blin >= 0))[0][:8].tolist()}"
    assert got.sum() > 50 and (~got).sum() > 20
    assert (np.abs(t - bt)[got] <= BOUND * np.maximum(np.abs(t), np.abs(bt))[got]).all()
    assert np.array_equal(hit, blin.astype(np.int32))
    assert (gap[got] == 0.0).sum() > 5                                                 # rays whose two earliest voxels are met at the same instant


def test_origin_inside_an_occupied_voxel_and_near_far():
    v = scene()
    lin = np.nonzero(SR.occupied(v).reshape(-1))[0][::7]
    c = np.stack(np.unravel_index(lin, SHAPE), axis=1).astype(np.float64)
    rng = np.random.default_rng(3)
    o = LO + (c + rng.uniform(0.1, 0.9, size=c.shape)) * S
    d = rng.normal(size=c.shape)
    t, hit, face, _ = SR.walk(v, LO, S, o, d, 0.0, FAR)
    assert np.array_equal(hit, lin.astype(np.int32)) and (t == 0.0).all() and (face == SR.FACE_NEAR).all()
    compare("inside", o, d)
    # near inside a wall: the ray starts in the floor's depth; far short of it: a miss
    o2 = np.tile(LO + np.array([9.5, 6.5, 10.5]) * S, (2, 1))
    d2 = np.array([[0.0, -1.0, 0.0], [0.01, -1.0, 0.02]])
    t, hit, face, _ = SR.walk(np.where(np.arange(9)[None, :, None] == 0, v, np.uint32(0xFF000000)), LO, S, o2, d2, 6.2 * S, FAR)
    assert (face == SR.FACE_NEAR).all() and (t == 6.2 * S).all() and (hit >= 0).all()
    t, hit, face, _ = SR.walk(np.where(np.arange(9)[None, :, None] == 0, v, np.uint32(0xFF000000)), LO, S, o2, d2, 0.0, 5.0 * S)
    assert (hit == -1).all() and (t == -1.0).all()


def test_origins_outside_every_face():
    ext = np.asarray(SHAPE) * S
    rng = np.random.default_rng(8)
    o, d = [], []
    for a in range(3):
        for side in (-1, 1):
            p = LO + rng.uniform(0.1, 0.9, size=(60, 3)) * ext
            p[:, a] = LO[a] + (ext[a] * (side > 0)) + side * rng.uniform(0.01, 0.5, size=60)
            target = LO + rng.uniform(0.0, 1.0, size=(60, 3)) * ext
            o.append(p)
            d.append(target - p)
    assert compare("outside", np.concatenate(o), np.concatenate(d)) > 100
    # pointing away, or parallel to a face beside the grid: misses
    t, hit, _, _ = SR.walk(scene(), LO, S, np.array([LO - 0.1, LO - 0.1]), np.array([[-1.0, -1.0, -1.0], [0.0, 1.0, 0.0]]), NEAR, FAR)
    assert (hit == -1).all()


def test_rays_that_are_not_finite_are_counted():
    o = np.array([[0.0, 0.0, 1.0], [np.nan, 0.0, 1.0], [0.0, 0.0, 1.0]])
    d = np.array([[0.0, -1.0, 0.0], [0.0, -1.0, 0.0], [np.inf, 0.0, 0.0]])
    t, hit, face, bad = SR.walk(scene(), LO, S, o, d, NEAR, FAR)
    assert bad.tolist() == [False, True, True] and (hit[1:] == -1).all()


def test_views_shade_and_pack():
    v = scene()
    c2w = np.array([[[1.0, 0, 0, -0.8], [0, 1.0, 0, 0.1], [0, 0, 1.0, 1.5]]])
    r = SR.views(v, LO, S, c2w, 9, 7, 4.5, 0.0, 50.0)
    hit = r["hit"] >= 0
    assert hit.any() and (~hit).any()
    assert (r["rgba"][..., 3] == 255).all() and (r["rgba"][~hit][:, :3] == 0).all() and (r["depth"][~hit] == 0).all() and (r["sem"][~hit] == 0).all()
    y, x = np.argwhere(hit[0])[0]
    w = int(v.reshape(-1)[r["hit"][0, y, x]])
    k = int(SR.SHADE[r["face"][0, y, x]])
    assert r["rgba"][0, y, x].tolist() == [((w & 255) * k + 127) // 255, (((w >> 8) & 255) * k + 127) // 255, (((w >> 16) & 255) * k + 127) // 255, 255]
    assert r["sem"][0, y, x] == w >> 24 and r["info"][0] == (~hit).sum()
    ray = SR.views(v, LO, S, c2w, 9, 7, 4.5, 0.0, 50.0, ray_depth=True)
    assert (ray["depth64"][hit] >= r["depth64"][hit]).all() and ray["depth64"][0, 3, 4] == r["depth64"][0, 3, 4]      # the centre pixel: cam = (0, 0, -1)


def test_brick_mask_restatement():
    v = SR.clutter_grid((70, 9, 40), 0.002, 2, floor=False)
    words = SR.build_bricks(v)
    assert words.shape[0] == SR.bricks_words(v.shape) == 4 and words.shape[0] % 2 == 0       # 9 x 2 x 5 = 90 bricks: three words, rounded up to even
    for x, y, z in np.argwhere(SR.occupied(v)):
        b = ((x >> 3) * 2 + (y >> 3)) * 5 + (z >> 3)
        assert (words[b >> 5] >> np.uint32(b & 31)) & 1
    assert sum(bin(int(w)).count("1") for w in words) == len({(x >> 3, y >> 3, z >> 3) for x, y, z in np.argwhere(SR.occupied(v))})


# ------------------------------------------------------------------ the builders' host halves
def test_from_occupancy_classes_are_the_standins_hash():
    """The class of every voxel is analytic_targets' formula (standin.py:55-57) at the voxel's centre, in its float32 torch arithmetic."""
    import torch
    from apnrf_amd import sensor as SN
    from apnrf_amd import synthetic as S
    aabb = np.array([-2.0, -0.2, -1.0, 0.0, 1.0, 1.4], np.float32)
    res = S.grid_resolution(aabb)
    occ = S.make_occupancy(res, seed=3, clutter=0.1)
    words, lo, s = SN.occupancy_words(occ, aabb, cell=0.2, refine=4, num_classes=29)
    assert words.shape == tuple(4 * n for n in res) and s == 0.05 and words.dtype == np.uint32
    fine = np.repeat(np.repeat(np.repeat(occ[0], 4, 0), 4, 1), 4, 2)
    assert np.array_equal((words >> 24) != 0xFF, fine)
    idx = np.argwhere(fine)
    p = torch.from_numpy((lo + (idx + 0.5) * s).astype(np.float32))
    a = torch.as_tensor(aabb, dtype=torch.float32)
    cell = torch.floor((p - a[:3]) / 0.2).to(torch.int64)
    label = ((cell[:, 0] * 73856093) ^ (cell[:, 1] * 19349663) ^ (cell[:, 2] * 83492791)) % 29
    assert np.array_equal((words[fine] >> 24).astype(np.int64), label.numpy())
    assert np.array_equal(label.numpy(), SR.cell_hash(idx[:, 0] // 4, idx[:, 1] // 4, idx[:, 2] // 4))
    # colour: fract of the centre, one byte per axis
    c = lo + (idx + 0.5) * s
    want = np.minimum(np.floor((c - np.floor(c)) * 256.0), 255).astype(np.uint32)
    got = words[fine]
    assert np.array_equal(np.stack([got & 255, (got >> 8) & 255, (got >> 16) & 255], 1), want)
    assert (words[~fine] == 0xFF000000).all()
    # closed: the six outer faces, nothing else
    closed, _, _ = SN.occupancy_words(occ, aabb, refine=1, closed=True)
    o = (closed >> 24) != 0xFF
    assert o[0].all() and o[-1].all() and o[:, 0].all() and o[:, -1].all() and o[:, :, 0].all() and o[:, :, -1].all()
    assert np.array_equal(o[1:-1, 1:-1, 1:-1], occ[0][1:-1, 1:-1, 1:-1])


def test_from_point_cloud_lowest_index_wins():
    from apnrf_amd import sensor as SN
    rng = np.random.default_rng(4)
    pts = rng.uniform(-0.4, 0.9, size=(500, 3))
    col = rng.integers(0, 256, size=(500, 3)).astype(np.uint8)
    lab = rng.integers(0, 29, size=500)
    words, lo, s = SN.point_cloud_words(pts, col, lab, 0.1)
    assert np.array_equal(lo, pts.min(axis=0))
    cells, first = SR.first_point_wins(pts, lo, 0.1, words.shape)
    assert len(cells) < 500                                                            # several points share a voxel: the rule is exercised
    flat = words.reshape(-1)
    assert np.array_equal(np.nonzero((flat >> 24) != 0xFF)[0], cells)
    assert np.array_equal(flat[cells], SR.pack(col[first, 0], col[first, 1], col[first, 2], lab[first]))
    with pytest.raises(ValueError):
        SN.point_cloud_words(pts, col, np.full(500, 255), 0.1)
    # no colours, no labels, a given corner
    w2, lo2, _ = SN.point_cloud_words(pts, None, None, 0.1, lo=[-0.5, -0.5, -0.5])
    assert (w2.reshape(-1)[(w2.reshape(-1) >> 24) != 0xFF] == SR.pack(128, 128, 128, 0)).all() and lo2.tolist() == [-0.5, -0.5, -0.5]
