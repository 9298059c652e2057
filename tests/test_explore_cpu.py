"""CPU-side checks of the exploration map (csrc/explore.hip, apnrf_amd/explore.py): the seven symbols are declared, exported and bound; every
argument error is refused with MNF_ERR_INVALID before anything touches a device; and the numpy restatement the GPU tests compare against
(tests/explore_ref.py) is itself held to what the definition promises: walks of exactly sum(n_k) steps that end in b and stay on the exact
float64 segment, frontier multiplicities worked by hand, clusters equal to scikit-learn's DBSCAN both on the duplicated list and with
sample_weight, and goal ties that go to the lowest cell."""
import ctypes
import os
import re

import numpy as np
import pytest

import apnrf_amd
from apnrf_amd import _lib as L

import explore_ref as ER

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("mnf_explore_map_bytes", "mnf_explore_map_insert", "mnf_explore_map_count", "mnf_explore_map_topdown", "mnf_explore_map_frontiers",
           "mnf_explore_map_frontier_clusters_workspace_bytes", "mnf_explore_map_frontier_clusters")
INVALID = -1


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as G
    G.build()
    return apnrf_amd.load_library()


# ------------------------------------------------------------------ the boundary
def test_symbols_declared_exported_and_bound(lib):
    header = open(os.path.join(REPO, "include", "mi355nerf.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    raw = ctypes.CDLL(L.lib_path())
    for s in SYMBOLS:
        assert re.search(r"\b" + s + r"\s*\(", code), f"{s} is not declared in include/mi355nerf.h"
        assert hasattr(raw, s), f"{s} is not exported"
        assert s in L.SIGNATURES
    assert L.SIGNATURES["mnf_explore_map_bytes"][0] is ctypes.c_int64
    assert L.SIGNATURES["mnf_explore_map_frontier_clusters_workspace_bytes"][0] is ctypes.c_int64
    assert header.count("typedef struct {") == 5                             # plain arguments: no new struct
    assert "frontier_baseline.py" in header and ":52-67" in header and ":191-214" in header
    assert lib.mnf_version() == 1
    from apnrf_amd import explore
    assert hasattr(explore, "ExplorationMap") and hasattr(explore, "next_goal")
    with pytest.raises(L.MnfError):
        explore.ExplorationMap([0, 0, 0, 1, 1, 1], device="cpu")             # no CPU fallback


def test_byte_functions(lib):
    assert lib.mnf_explore_map_bytes(16, 8, 16) == 2 * 64 * 4                       # 2048 voxels: 64 words, already even
    assert lib.mnf_explore_map_bytes(7, 5, 9) == 2 * 10 * 4                         # 315 voxels: 10 words
    assert lib.mnf_explore_map_bytes(3, 3, 3) == 2 * 2 * 4                          # 27 voxels: 1 word, padded to 2 (8-byte planes)
    assert lib.mnf_explore_map_bytes(1, 1, 1) == 16
    for res in [(16, 8, 16), (7, 5, 9), (3, 3, 3), (1, 1, 1)]:
        assert lib.mnf_explore_map_bytes(*res) == 2 * ER.words_per_plane(res) * 4
        assert lib.mnf_explore_map_bytes(*res) == 2 * lib.mnf_object_map_bytes(1, *res)            # the object map's plane
    for bad in [(0, 4, 4), (-1, 4, 4), (4, 0, 4), (4, -3, 4), (4, 4, 0), (2048, 2048, 2048), ((1 << 24) + 1, 1, 1)]:
        assert lib.mnf_explore_map_bytes(*bad) == 0, bad
        assert lib.mnf_object_map_bytes(1, *bad) == 0, bad                                          # the same geometries are refused
    ws = lib.mnf_explore_map_frontier_clusters_workspace_bytes
    a, b, c = ws(16, 16, 0, 0), ws(16, 16, 100, 10), ws(16, 16, 1000, 10)
    assert 0 < a < b < c and a % 8 == 0 and b % 8 == 0 and c % 8 == 0
    assert ws(16, 16, 100, 10) < ws(16, 16, 100, 20) and ws(16, 16, 100, 10) < ws(16, 32, 100, 10)
    for bad in [(0, 4, 10, 10), (4, 0, 10, 10), (4, 4, -1, 10), (4, 4, 10, -1), (-4, 4, 10, 10)]:
        assert ws(*bad) == 0, bad
    # the layout, byte for byte: no capacity, counts that need padding to 8 bytes, a realistic map
    pinned = {(16, 16, 0, 0): 1048, (16, 16, 100, 10): 3568, (16, 16, 1000, 10): 25168, (7, 9, 0, 0): 280, (7, 9, 33, 5): 1144, (7, 9, 33, 0): 1080,
              (1, 1, 1, 1): 80, (196, 196, 38416, 38416): 1536808, (196, 196, 5001, 333): 277736}
    for args, want in pinned.items():
        assert ws(*args) == want, args


GMIN = (ctypes.c_float * 3)(0.0, 0.0, 0.0)


def _insert(lib, **over):
    """mnf_explore_map_insert with plausible (never dereferenced) device pointers; `over` replaces arguments by name."""
    a = dict(bits=0x1000, res_x=7, res_y=5, res_z=9, grid_min=GMIN, voxel_size=0.1, max_range=10.0, origins=0x2000, viewdirs=0x3000, depth=0x4000,
             acc=None, n_rays=64, min_depth=0.0, min_acc=0.0, stats=None, stream=None)
    a.update(over)
    rc = lib.mnf_explore_map_insert(*a.values())
    return rc, lib.mnf_last_error().decode()


def _clusters(lib, **over):
    a = dict(cells=0x1000, mult=0x2000, frontier_info=0x3000, max_frontiers=100, res_x=7, res_z=9, eps2=1, min_samples=3, weighted=1, current_x=1.0,
             current_z=2.0, max_clusters=50, labels=0x4000, goals=0x5000, sizes=0x6000, info=0x7000, workspace=0x10000, workspace_bytes=None, stream=None)
    a.update(over)
    if a["workspace_bytes"] is None:
        a["workspace_bytes"] = lib.mnf_explore_map_frontier_clusters_workspace_bytes(a["res_x"], a["res_z"], max(a["max_frontiers"], 0),
                                                                                     max(a["max_clusters"], 0))
    rc = lib.mnf_explore_map_frontier_clusters(*a.values())
    return rc, lib.mnf_last_error().decode()


@pytest.mark.parametrize("name", ["bits", "origins", "viewdirs", "depth", "grid_min"])
def test_insert_refuses_null_required_pointer(lib, name):
    rc, msg = _insert(lib, **{name: None})
    assert rc == INVALID and name in msg, (rc, msg)


def test_insert_refuses_bad_arguments(lib):
    inf, nan = float("inf"), float("nan")
    for over, word in [(dict(res_x=0), "resolution"), (dict(res_y=-2), "resolution"), (dict(res_z=0), "resolution"), (dict(voxel_size=0.0), "voxel_size"),
                       (dict(voxel_size=-0.1), "voxel_size"), (dict(voxel_size=nan), "voxel_size"), (dict(voxel_size=inf), "voxel_size"),
                       (dict(max_range=0.0), "max_range"), (dict(max_range=-1.0), "max_range"), (dict(max_range=inf), "max_range"),
                       (dict(max_range=nan), "max_range"), (dict(max_range=1.0e6, voxel_size=0.5), "2^20"),
                       (dict(max_range=float(2 ** 20 + 1), voxel_size=1.0), "2^20"), (dict(n_rays=-1), "n_rays"), (dict(min_depth=nan), "NaN"),
                       (dict(min_acc=nan), "NaN"), (dict(bits=0x1004), "aligned"), (dict(stats=0x8004), "aligned"),
                       (dict(res_x=2048, res_y=2048, res_z=2048), "indexes")]:
        rc, msg = _insert(lib, **over)
        assert rc == INVALID and word in msg, (over, rc, msg)


def test_insert_of_nothing_is_ok(lib):
    rc, _ = _insert(lib, n_rays=0, bits=None, origins=None, viewdirs=None, depth=None)
    assert rc == 0
    rc, _ = _insert(lib, n_rays=0)
    assert rc == 0


def test_read_outs_refuse_bad_arguments(lib):
    assert lib.mnf_explore_map_count(None, 7, 5, 9, 0x2000, None) == INVALID and b"bits" in lib.mnf_last_error()
    assert lib.mnf_explore_map_count(0x1000, 7, 5, 9, None, None) == INVALID and b"counts" in lib.mnf_last_error()
    assert lib.mnf_explore_map_count(0x1000, 0, 5, 9, 0x2000, None) == INVALID
    td = lib.mnf_explore_map_topdown
    assert td(None, 7, 5, 9, 0, 5, 0x2000, None) == INVALID and b"bits" in lib.mnf_last_error()
    assert td(0x1000, 7, 5, 9, 0, 5, None, None) == INVALID and b"map" in lib.mnf_last_error()
    for lo, hi in [(-1, 5), (0, 6), (3, 2), (6, 6)]:
        assert td(0x1000, 7, 5, 9, lo, hi, 0x2000, None) == INVALID and b"layers" in lib.mnf_last_error(), (lo, hi)
    assert td(0x1000, 7, -5, 9, 0, 5, 0x2000, None) == INVALID
    fr = lib.mnf_explore_map_frontiers
    assert fr(None, 7, 9, 10, 0x2000, 0x3000, 0x4000, None) == INVALID and b"map" in lib.mnf_last_error()
    assert fr(0x1000, 7, 9, 10, None, 0x3000, 0x4000, None) == INVALID and b"cells" in lib.mnf_last_error()
    assert fr(0x1000, 7, 9, 10, 0x2000, None, 0x4000, None) == INVALID and b"mult" in lib.mnf_last_error()
    assert fr(0x1000, 7, 9, 10, 0x2000, 0x3000, None, None) == INVALID and b"info" in lib.mnf_last_error()
    assert fr(0x1000, 7, 9, -1, 0x2000, 0x3000, 0x4000, None) == INVALID and b"max_frontiers" in lib.mnf_last_error()
    assert fr(0x1000, 0, 9, 10, 0x2000, 0x3000, 0x4000, None) == INVALID and b"geometry" in lib.mnf_last_error()


@pytest.mark.parametrize("name", ["cells", "mult", "frontier_info", "labels", "goals", "sizes", "info", "workspace"])
def test_clusters_refuses_null_required_pointer(lib, name):
    rc, msg = _clusters(lib, **{name: None})
    assert rc == INVALID and name in msg, (rc, msg)


def test_clusters_refuses_bad_arguments(lib):
    for over, word in [(dict(res_x=0), "geometry"), (dict(res_z=-1), "geometry"), (dict(eps2=0), "eps2"), (dict(eps2=9), "eps2"), (dict(eps2=-1), "eps2"),
                       (dict(min_samples=0), "min_samples"), (dict(max_frontiers=-1, workspace_bytes=1 << 20), "max_frontiers"),
                       (dict(max_clusters=-1, workspace_bytes=1 << 20), "max_clusters"), (dict(current_x=float("nan")), "current"),
                       (dict(current_z=float("inf")), "current"), (dict(workspace=0x10004), "aligned")]:
        rc, msg = _clusters(lib, **over)
        assert rc == INVALID and word in msg, (over, rc, msg)
    need = lib.mnf_explore_map_frontier_clusters_workspace_bytes(7, 9, 100, 50)
    for small in (need - 1, 0):
        rc, msg = _clusters(lib, workspace_bytes=small)
        assert rc == INVALID and "workspace too small" in msg, (rc, msg)


# ------------------------------------------------------------------ the walk
def _box_meets_segment(lo, hi, p0, p1):
    """Exact slab test in float64: does the segment p0 -> p1 meet the box [lo, hi]?"""
    t0, t1 = 0.0, 1.0
    for k in range(3):
        dk = p1[k] - p0[k]
        if dk == 0.0:
            if p0[k] < lo[k] or p0[k] > hi[k]:
                return False
            continue
        ta, tb = (lo[k] - p0[k]) / dk, (hi[k] - p0[k]) / dk
        if ta > tb:
            ta, tb = tb, ta
        t0, t1 = max(t0, ta), min(t1, tb)
        if t0 > t1:
            return False
    return True


@pytest.fixture(scope="module")
def walked():
    case = ER.seeded_rays(ER.RES_A, 1000, 5)
    setup = ER.ray_setup(case["o"], case["d"], case["depth"], ER.G_MIN, ER.G_VS, ER.MAX_RANGE, acc=case["acc"], min_depth=ER.MIN_DEPTH, min_acc=ER.MIN_ACC)
    return case, setup, ER.paths(setup)


def test_walk_has_exactly_sum_n_steps_and_ends_in_b(walked):
    case, setup, paths = walked
    keep = setup["keep"]
    assert 300 < keep.sum() < 1000 and len(paths) == keep.sum()
    for i, path in paths.items():
        assert len(path) == int(setup["n"][i].sum()) + 1, i
        assert path[0] == tuple(setup["a"][i]) and path[-1] == tuple(setup["b"][i]), i
        steps = np.abs(np.diff(np.array(path), axis=0))
        assert steps.size == 0 or ((steps.sum(axis=1) == 1).all() and steps.max() == 1), i       # one axis, one voxel at a time
    # the fixture holds what it promises
    n = setup["n"][keep]
    res = np.array(ER.RES_A)
    a, b = setup["a"][keep], setup["b"][keep]
    assert (n.sum(axis=1) == 0).sum() > 10                                                       # a == b
    assert ((n > 0).sum(axis=1) == 1).sum() > 20                                                 # axis-parallel
    assert (((a < 0) | (a >= res)).any(axis=1)).sum() > 20                                       # origins outside the grid
    assert (((b < 0) | (b >= res)).any(axis=1)).sum() > 20                                       # end points outside the grid
    assert (~setup["hit"][keep]).sum() > 20
    # skipped: NaN, <= min_depth, acc below, non-finite or huge rays; kept: +inf and beyond max_range (as misses), NaN acc
    dep, acc = case["depth"], case["acc"]
    assert not keep[np.isnan(dep)].any() and not keep[dep <= ER.MIN_DEPTH].any() and not keep[acc < ER.MIN_ACC].any()
    assert not keep[~np.isfinite(case["o"]).all(axis=1) | ~np.isfinite(case["d"]).all(axis=1)].any()
    assert keep[np.isposinf(dep)].any() and not setup["hit"][np.isposinf(dep)].any()
    assert keep[np.isnan(acc) & (dep > 1.0) & (np.arange(len(dep)) > 400)].any()


def test_walk_stays_on_the_exact_segment(walked):
    """Every visited voxel box, enlarged by 1 % of a voxel on each side, meets the float64 segment o -> o + t d."""
    case, setup, paths = walked
    g, vs = np.asarray(ER.G_MIN, np.float32).astype(np.float64), float(np.float32(ER.G_VS))
    checked = 0
    for i, path in paths.items():
        p0 = case["o"][i].astype(np.float64)
        p1 = p0 + float(setup["t"][i]) * case["d"][i].astype(np.float64)
        for v in path:
            lo = g + (np.array(v, np.float64) - 0.01) * vs
            hi = g + (np.array(v, np.float64) + 1.01) * vs
            assert _box_meets_segment(lo, hi, p0, p1), (i, v)
            checked += 1
    assert checked > 3000


def test_diagonal_ties_take_x_then_y_then_z():
    """From a voxel centre along (1, -1, 1): all three tm tie at every corner, so the walk steps x, then y, then z, again and again."""
    lo = np.array(ER.G_MIN, np.float32)
    o = lo + (np.array([2, 6, 3], np.float32) + np.float32(0.5)) * np.float32(ER.G_VS)
    setup = ER.ray_setup(o[None], np.array([[1, -1, 1]], np.float32), [0.5], ER.G_MIN, ER.G_VS, ER.MAX_RANGE)
    assert setup["tm"][0].tolist() == [0.125, 0.125, 0.125] and setup["n"][0].tolist() == [2, 2, 2]
    assert ER.paths(setup)[0] == [(2, 6, 3), (3, 6, 3), (3, 5, 3), (3, 5, 4), (4, 5, 4), (4, 4, 4), (4, 4, 5)]


def test_insert_restatement_hand_worked():
    """A 4 x 4 x 4 grid of 0.5 m voxels at the origin, rays from (0.25, 0.25, 0.25) along +x."""
    res, o, d = (4, 4, 4), [[0.25, 0.25, 0.25]], [[1.0, 0.0, 0.0]]
    # voxel (x, 0, 0) is bit 16 x of the plane: x = 0, 1 in word 0, x = 2, 3 in word 1
    hit = ER.insert(ER.new_bits(res), o, d, [1.0], (0, 0, 0), 0.5, res, 3.0)                      # ends in voxel 2: 0 and 1 free, 2 occupied
    assert hit[0].tolist() == [1 | 1 << 16, 0] and hit[1].tolist() == [0, 1]
    miss = ER.insert(ER.new_bits(res), o, d, [np.inf], (0, 0, 0), 0.5, res, 1.0)                  # carves to max_range (voxel 2), marks nothing
    assert miss[0].tolist() == [1 | 1 << 16, 1] and not miss[1].any()
    out = ER.insert(ER.new_bits(res), o, d, [2.0], (0, 0, 0), 0.5, res, 3.0)                      # ends outside: four free voxels, none occupied
    assert ER.counts(out, res).tolist() == [4, 0, 60]
    both = ER.insert(hit.copy(), o, d, [1.5], (0, 0, 0), 0.5, res, 3.0)                           # a later ray passes through the occupied voxel
    st = ER.voxel_states(both, res)
    assert st[2, 0, 0] == 1 and st[3, 0, 0] == 1 and st[1, 0, 0] == 0 and ER.counts(both, res).tolist() == [2, 2, 60]
    assert ER.top_down(both, res)[:, 0].tolist() == [0, 0, 1, 1] and (ER.top_down(both, res)[:, 1:] == -1).all()
    assert (ER.top_down(both, res, 1, 4) == -1).all() and (ER.top_down(both, res, 2, 2) == -1).all()


# ------------------------------------------------------------------ frontier multiplicities, by hand
U, F, O = -1, 0, 1
HAND_MAPS = {
    # one unknown cell in the middle of free space: the eight cells around it; those in its own column x see it at dx = 0 only, the columns
    # beside it at dx = -1 or +1 only: everything has multiplicity 1
    "hole": ([[F, F, F, F, F], [F, F, F, F, F], [F, F, U, F, F], [F, F, F, F, F], [F, F, F, F, F]],
             {(1, 1): 1, (1, 2): 1, (1, 3): 1, (2, 1): 1, (2, 3): 1, (3, 1): 1, (3, 2): 1, (3, 3): 1}),
    # an unknown row x = 0 above free rows: each cell of row 1 sees unknowns only in the column dx = -1: once
    "edge_row": ([[U, U, U, U, U], [F, F, F, F, F], [F, F, F, F, F], [F, F, F, F, F], [F, F, F, F, F]],
                 {(1, 0): 1, (1, 1): 1, (1, 2): 1, (1, 3): 1, (1, 4): 1}),
    # an unknown column z = 0 beside free columns: each cell of column 1 sees an unknown at every dx that is inside the map: 2 at the two ends, 3 between
    "edge_column": ([[U, F, F, F, F], [U, F, F, F, F], [U, F, F, F, F], [U, F, F, F, F], [U, F, F, F, F]],
                    {(0, 1): 2, (1, 1): 3, (2, 1): 3, (3, 1): 3, (4, 1): 2}),
    # a single free cell in the unknown: all three columns, its own included (above and below it)
    "island": ([[U, U, U, U, U], [U, U, U, U, U], [U, U, F, U, U], [U, U, U, U, U], [U, U, U, U, U]], {(2, 2): 3}),
    # ... and in a corner of the map: dx = -1 is outside
    "corner": ([[F, U, U, U, U], [U, U, U, U, U], [U, U, U, U, U], [U, U, U, U, U], [U, U, U, U, F]], {(0, 0): 2, (4, 4): 2}),
    # occupied cells are neither frontier cells nor unknown neighbours; (2, 2) is walled off from the unknown column but for the gap at (3, 1) ... which
    # is not adjacent to an unknown itself
    "walls": ([[U, O, F, F, F], [U, O, F, F, F], [U, O, F, F, F], [U, F, F, F, F], [U, O, F, F, F]], {(3, 1): 3}),
    "none_free": ([[F] * 5] * 5, {}),
    "none_unknown": ([[U] * 5] * 5, {}),
}


@pytest.mark.parametrize("name", list(HAND_MAPS))
def test_frontier_multiplicities_hand_worked(name):
    grid, want = HAND_MAPS[name]
    cells, mult, info = ER.frontiers(np.array(grid, np.int8))
    got = {(int(x), int(z)): int(m) for (x, z), m in zip(cells, mult)}
    assert got == want
    assert [tuple(c) for c in cells.tolist()] == sorted(want)                                    # ascending x * Z + z
    assert info.tolist() == [len(want), 0]
    if len(want) > 1:
        cut = ER.frontiers(np.array(grid, np.int8), max_frontiers=len(want) - 1)
        assert cut[2].tolist() == [len(want), 1] and cut[0].shape[0] == len(want) - 1 == cut[1].shape[0]


# ------------------------------------------------------------------ clusters against scikit-learn
def _from_grid(grid):
    cells, mult, _ = ER.frontiers(grid)
    return cells, mult


def _border_column():
    """An unknown column with a wall cell in it: the frontier cell beside the wall cell and its two neighbours are listed twice (one of their three
    columns holds no unknown), the cells further along three times, the two at the ends of the map twice."""
    g = np.zeros((7, 6), np.int8)
    g[:, 0] = U
    g[3, 0] = O                                                      # (3, 1) sees unknowns at dx = -1 and +1 only
    g[:, 3] = O
    g[5, 5] = U                                                      # a second, small group on the far side
    return g


CLUSTER_CASES = {"border": lambda: (ER.BORDER_CELLS, np.ones(len(ER.BORDER_CELLS), np.int32)),
                 "border_weights": lambda: (ER.BORDER_CELLS, np.array([1, 2, 3, 1, 1, 2, 3, 1, 2], np.int32)),
                 "column": lambda: _from_grid(_border_column()), **{f"seed{s}": (lambda s=s: _from_grid(ER.seeded_map2d(s))) for s in range(12)},
                 "big": lambda: _from_grid(ER.seeded_map2d(99, (40, 33), (0.2, 0.6, 0.2)))}


@pytest.mark.parametrize("weighted", [True, False])
@pytest.mark.parametrize("eps2", [1, 2, 4])
@pytest.mark.parametrize("case", list(CLUSTER_CASES))
def test_clusters_match_sklearn_dbscan(case, eps2, weighted):
    """eps: any value with eps2 <= eps^2 < eps2 + 1 links exactly the integer offsets with dx^2 + dz^2 <= eps2; sqrt(eps2 + 0.5) is one that
    no rounding of a distance can move across."""
    cluster = pytest.importorskip("sklearn.cluster")
    cells, mult = CLUSTER_CASES[case]()
    assert cells.shape[0] > 3
    eps = float(np.sqrt(eps2 + 0.5))
    for min_samples in (3, 4, 6):
        ref = ER.frontier_clusters(cells, mult, (0.0, 0.0), eps2=eps2, min_samples=min_samples, weighted=weighted)
        pts = cells.astype(np.float64)
        what = f"{case} eps2={eps2} min_samples={min_samples}"
        if weighted:
            by_weight = cluster.DBSCAN(eps=eps, min_samples=min_samples).fit_predict(pts, sample_weight=mult.astype(np.float64))
            np.testing.assert_array_equal(ref["labels"], by_weight, err_msg=what + " sample_weight")
            dup = np.repeat(np.arange(len(cells)), mult)                                         # the reference's list: each cell mult times, in order
            by_dup = cluster.DBSCAN(eps=eps, min_samples=min_samples).fit_predict(pts[dup])
            np.testing.assert_array_equal(ref["labels"][dup], by_dup, err_msg=what + " duplicated")
        else:
            plain = cluster.DBSCAN(eps=eps, min_samples=min_samples).fit_predict(pts)
            np.testing.assert_array_equal(ref["labels"], plain, err_msg=what + " unweighted")
        K = int(ref["info"][0])
        assert K == ref["labels"].max() + 1 and ref["sizes"].tolist() == np.bincount(ref["labels"][ref["labels"] >= 0], minlength=K).tolist()


def test_border_cell_between_two_clusters_takes_the_smaller_label():
    cells = ER.BORDER_CELLS
    ref = ER.frontier_clusters(cells, np.ones(len(cells), np.int32), (0.0, 0.0), eps2=1, min_samples=4, weighted=False)
    assert ref["labels"].tolist() == ER.BORDER_LABELS and ref["info"].tolist() == [2, 0] and ref["sizes"].tolist() == [5, 4]
    assert ref["labels"][cells.tolist().index([2, 3])] == 0          # the shared arm: a neighbour of both centres, core of neither
    heavy = np.ones(len(cells), np.int32)
    heavy[cells.tolist().index([2, 3])] = 3                          # listed three times, the shared arm is core (3 + 2 >= 4) and joins the two
    ref = ER.frontier_clusters(cells, heavy, (0.0, 0.0), eps2=1, min_samples=4, weighted=True)
    assert ref["info"].tolist() == [1, 0] and (ref["labels"] == 0).all()
    cells, mult = _from_grid(_border_column())
    assert mult[cells.tolist().index([3, 1])] == 2 and mult[cells.tolist().index([2, 1])] == 2 and mult[cells.tolist().index([1, 1])] == 3
    assert mult[cells.tolist().index([0, 1])] == 2


def test_goal_is_the_nearest_member_and_ties_go_to_the_lowest_cell():
    cells = np.array([[2, 2], [2, 3], [2, 4], [3, 4], [4, 4], [8, 8], [8, 9], [9, 8]], np.int32)
    mult = np.ones(8, np.int32)
    ref = ER.frontier_clusters(cells, mult, (3.0, 3.0), eps2=1, min_samples=2, weighted=True)
    assert ref["labels"].tolist() == [0, 0, 0, 0, 0, 1, 1, 1] and ref["sizes"].tolist() == [5, 3]
    assert ref["goals"].tolist() == [[2, 3], [8, 8]]                 # (2, 3) and (3, 4) are both 1 away: the lower row-major cell
    ref = ER.frontier_clusters(cells, mult, (3.0, 3.5), eps2=1, min_samples=2, weighted=True)
    assert ref["goals"].tolist() == [[3, 4], [8, 8]]
    ref = ER.frontier_clusters(cells, mult, (8.5, 8.5), eps2=1, min_samples=2, weighted=True)
    assert ref["goals"].tolist() == [[4, 4], [8, 8]]                 # (8, 8), (8, 9), (9, 8) tie at 0.5: the lowest
    capped = ER.frontier_clusters(cells, mult, (8.5, 8.5), eps2=1, min_samples=2, max_clusters=1)
    assert capped["info"].tolist() == [2, 1] and capped["goals"].tolist() == [[4, 4]] and capped["labels"].tolist() == ref["labels"].tolist()


def test_next_goal_helper():
    from apnrf_amd.explore import next_goal
    goals, cells = np.array([[5.0, 5.0], [1.0, 1.0], [2.0, 0.0]]), np.array([[50, 50], [10, 10], [20, 0]])
    visited = []
    g, order = next_goal(goals, cells, (0.0, 0.0), visited)
    assert g.tolist() == [1.0, 1.0] and order.tolist() == [1, 2, 0] and visited == [(10, 10)]
    g, order = next_goal(goals, cells, (0.0, 0.0), visited)
    assert g.tolist() == [2.0, 0.0] and order.tolist() == [2, 0] and visited == [(10, 10), (20, 0)]
    visited.append((50, 50))
    g, order = next_goal(goals, cells, (0.0, 0.0), visited)
    assert g is None and order.size == 0
