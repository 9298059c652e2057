"""CPU-side checks of the semantic object map (csrc/objmap.hip, apnrf_amd/objects.py): the six symbols are declared, exported and bound;
every argument error is refused with MNF_ERR_INVALID before anything touches a device; the numpy restatement the GPU tests compare against
(tests/objmap_ref.py) is itself held against two independent clusterings (sklearn's DBSCAN and scipy's cKDTree + connected_components) on
integer coordinates; the reason for defining linkage on integer offsets is asserted; and the greedy match is checked on hand-worked cases."""
import ctypes
import os
import re

import numpy as np
import pytest

import apnrf_amd
from apnrf_amd import _lib as L

import objmap_ref as OR

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("mnf_object_map_bytes", "mnf_object_map_insert", "mnf_object_map_count", "mnf_object_map_clusters_workspace_bytes",
           "mnf_object_map_clusters", "mnf_object_map_match")
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
    assert L.SIGNATURES["mnf_object_map_bytes"][0] is ctypes.c_int64
    assert L.SIGNATURES["mnf_object_map_clusters_workspace_bytes"][0] is ctypes.c_int64
    assert header.count("typedef struct {") == 5                             # plain arguments: no new struct
    assert "eval_pipeline_offline.py:119-138" in header and "eval_pipeline_offline.py:26-42" in header and "eval_pipeline_offline.py:45-70" in header
    assert lib.mnf_version() == 1
    from apnrf_amd import objects
    assert hasattr(objects, "SemanticObjectMap")


def test_byte_functions(lib):
    assert lib.mnf_object_map_bytes(29, 16, 8, 16) == 29 * 64 * 4                   # 2048 voxels: 64 words, already even
    assert lib.mnf_object_map_bytes(5, 7, 5, 9) == 5 * 10 * 4                       # 315 voxels: 10 words
    assert lib.mnf_object_map_bytes(3, 3, 3, 3) == 3 * 2 * 4                        # 27 voxels: 1 word, padded to 2 (8-byte planes)
    assert lib.mnf_object_map_bytes(1, 1, 1, 1) == 8
    assert lib.mnf_object_map_bytes(29, 16, 8, 16) % 8 == 0 and lib.mnf_object_map_bytes(5, 7, 5, 9) // 5 % 8 == 0
    assert lib.mnf_object_map_bytes(2, 16, 8, 16) < lib.mnf_object_map_bytes(3, 16, 8, 16) < lib.mnf_object_map_bytes(3, 17, 8, 16)
    for bad in [(0, 4, 4, 4), (-1, 4, 4, 4), (2, 0, 4, 4), (2, 4, -3, 4), (2, 4, 4, 0), (1, 2048, 2048, 2048)]:
        assert lib.mnf_object_map_bytes(*bad) == 0, bad
    ws = lib.mnf_object_map_clusters_workspace_bytes
    a, b, c = ws(5, 16, 8, 16, 0), ws(5, 16, 8, 16, 100), ws(5, 16, 8, 16, 1000)
    assert 0 < a < b < c and a % 8 == 0 and b % 8 == 0 and c % 8 == 0
    assert ws(5, 16, 8, 16, 100) < ws(6, 16, 8, 16, 100) < ws(6, 32, 8, 16, 100)
    for bad in [(0, 4, 4, 4, 10), (2, 0, 4, 4, 10), (2, 4, 4, 4, -1), (2, 4, 4, -4, 10)]:
        assert ws(*bad) == 0, bad
    # the layout, byte for byte: no capacity, counts that need padding to 8 bytes, a realistic map
    pinned = {(5, 16, 8, 16, 0): 5152, (5, 16, 8, 16, 100): 11952, (5, 16, 8, 16, 1000): 73152, (5, 7, 5, 9, 0): 832, (5, 7, 5, 9, 33): 3088,
              (3, 3, 3, 3, 7): 616, (1, 1, 1, 1, 1): 144, (29, 196, 34, 196, 50001): 22344280}
    for args, want in pinned.items():
        assert ws(*args) == want, args


GMIN = (ctypes.c_float * 3)(0.0, 0.0, 0.0)


def _insert(lib, **over):
    """mnf_object_map_insert with plausible (never dereferenced) device pointers; `over` replaces arguments by name."""
    a = dict(bits=0x1000, n_classes=5, res_x=7, res_y=5, res_z=9, grid_min=GMIN, voxel_size=0.1, first_class=1, origins=0x2000, viewdirs=0x3000,
             depth=0x4000, acc=None, sem=0x5000, labels=None, label_is_u8=0, n_rays=64, min_depth=0.0, max_depth=10.0, min_acc=0.0, stream=None)
    a.update(over)
    rc = lib.mnf_object_map_insert(*a.values())
    return rc, lib.mnf_last_error().decode()


def _clusters(lib, **over):
    a = dict(bits=0x1000, n_classes=5, res_x=7, res_y=5, res_z=9, grid_min=GMIN, voxel_size=0.1, link_r2=4, min_cluster_voxels=1, max_voxels=100,
             max_clusters=100, clusters=0x2000, cluster_counts=0x3000, info=0x4000, voxel_ids=None, voxel_cluster=None, workspace=0x10000,
             workspace_bytes=None, stream=None)
    a.update(over)
    if a["workspace_bytes"] is None:
        a["workspace_bytes"] = lib.mnf_object_map_clusters_workspace_bytes(a["n_classes"], a["res_x"], a["res_y"], a["res_z"], max(a["max_voxels"], 0))
    rc = lib.mnf_object_map_clusters(*a.values())
    return rc, lib.mnf_last_error().decode()


def _match(lib, **over):
    a = dict(clusters=0x1000, info=0x2000, max_clusters=10, n_classes=5, gt_locs=0x3000, gt_class=0x4000, n_gt=4, det_dist_thresh=1.0,
             detected=0x5000, match=0x6000, gt_match=0x7000, stream=None)
    a.update(over)
    rc = lib.mnf_object_map_match(*a.values())
    return rc, lib.mnf_last_error().decode()


@pytest.mark.parametrize("name", ["bits", "origins", "viewdirs", "depth", "grid_min"])
def test_insert_refuses_null_required_pointer(lib, name):
    rc, msg = _insert(lib, **{name: None})
    assert rc == INVALID and name in msg, (rc, msg)


def test_insert_refuses_bad_arguments(lib):
    for over, word in [(dict(res_x=0), "resolution"), (dict(res_y=-2), "resolution"), (dict(res_z=0), "resolution"), (dict(voxel_size=0.0), "voxel_size"),
                       (dict(voxel_size=-0.1), "voxel_size"), (dict(voxel_size=float("nan")), "voxel_size"), (dict(n_classes=0), "n_classes"),
                       (dict(first_class=-1), "first_class"), (dict(first_class=5), "first_class"), (dict(n_rays=-1), "n_rays"),
                       (dict(sem=0x5000, labels=0x6000), "both"), (dict(sem=None, labels=None), "neither"), (dict(bits=0x1004), "aligned")]:
        rc, msg = _insert(lib, **over)
        assert rc == INVALID and word in msg, (over, rc, msg)


def test_insert_of_nothing_is_ok(lib):
    rc, _ = _insert(lib, n_rays=0, bits=None, origins=None, viewdirs=None, depth=None, sem=None)
    assert rc == 0


@pytest.mark.parametrize("name", ["bits", "grid_min", "clusters", "cluster_counts", "info", "workspace"])
def test_clusters_refuses_null_required_pointer(lib, name):
    rc, msg = _clusters(lib, **{name: None})
    assert rc == INVALID and name in msg, (rc, msg)


def test_clusters_refuses_bad_arguments(lib):
    for over, word in [(dict(res_x=0), "resolution"), (dict(res_z=-1), "resolution"), (dict(voxel_size=0.0), "voxel_size"), (dict(link_r2=0), "link_r2"),
                       (dict(link_r2=9), "link_r2"), (dict(link_r2=-4), "link_r2"), (dict(min_cluster_voxels=0), "min_cluster_voxels"),
                       (dict(max_voxels=-1, workspace_bytes=1 << 20), "max_voxels"), (dict(max_clusters=-1), "max_clusters"),
                       (dict(workspace=0x10004), "aligned"), (dict(n_classes=0, workspace_bytes=1 << 20), "n_classes")]:
        rc, msg = _clusters(lib, **over)
        assert rc == INVALID and word in msg, (over, rc, msg)
    need = lib.mnf_object_map_clusters_workspace_bytes(5, 7, 5, 9, 100)
    for small in (need - 1, 0):
        rc, msg = _clusters(lib, workspace_bytes=small)
        assert rc == INVALID and "workspace too small" in msg, (rc, msg)


def test_count_and_match_refuse_bad_arguments(lib):
    assert lib.mnf_object_map_count(None, 5, 7, 5, 9, 0x2000, None) == INVALID and b"bits" in lib.mnf_last_error()
    assert lib.mnf_object_map_count(0x1000, 5, 7, 5, 9, None, None) == INVALID and b"counts" in lib.mnf_last_error()
    assert lib.mnf_object_map_count(0x1000, 5, 0, 5, 9, 0x2000, None) == INVALID
    for name in ("clusters", "info", "gt_locs", "gt_class", "detected", "match", "gt_match"):
        rc, msg = _match(lib, **{name: None})
        assert rc == INVALID and name in msg, (name, rc, msg)
    for over, word in [(dict(n_classes=0), "n_classes"), (dict(max_clusters=-1), "max_clusters"), (dict(n_gt=-1), "n_gt"),
                       (dict(det_dist_thresh=float("nan")), "det_dist_thresh")]:
        rc, msg = _match(lib, **over)
        assert rc == INVALID and word in msg, (over, rc, msg)


# ------------------------------------------------------------------ the restatement's clustering against two independent ones
RES, GRIDS, seeded_grid, snake_grid = OR.RES, OR.GRIDS, OR.seeded_grid, OR.snake_grid


def _canonical(labels):
    """Relabel by order of first appearance."""
    first = {}
    return np.array([first.setdefault(int(v), len(first)) for v in labels], np.int32)


def _rows_from_labels(ijk, labels, gmin, vs):
    rows = []
    for k in range(int(labels.max()) + 1 if labels.size else 0):
        pts = ijk[labels == k]
        rows.append([0.0, float(len(pts))] + [float(np.float32(gmin[a])) + (pts[:, a].astype(np.float64).sum() / len(pts) + 0.5) * float(np.float32(vs))
                                             for a in range(3)])
    return np.array(rows, np.float64).reshape(-1, 5)


def _check_against_labels(ref, ijk, labels, what):
    lab = _canonical(labels)
    np.testing.assert_array_equal(ref["voxel_cluster"], lab, err_msg=what)                       # the same partition, in the same order
    rows = _rows_from_labels(ijk, lab, (0.25, -1.5, 3.0), 0.1)
    np.testing.assert_array_equal(ref["rows"][:, 1], rows[:, 1], err_msg=what)                   # counts
    np.testing.assert_array_equal(ref["rows"][:, 2:], rows[:, 2:], err_msg=what)                 # centroids, bit for bit
    assert ref["info"][1] == rows.shape[0] == ref["cluster_counts"][0]


@pytest.mark.parametrize("grid", list(GRIDS))
@pytest.mark.parametrize("link_r2", range(1, 9))
def test_restatement_matches_kdtree_components(grid, link_r2):
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    from scipy.spatial import cKDTree
    occ = GRIDS[grid]()
    bits = OR.grid_to_bits(occ[None])
    ref = OR.clusters(bits, RES, (0.25, -1.5, 3.0), 0.1, link_r2=link_r2)
    ijk = np.argwhere(occ)                                           # ascending linear index
    pairs = cKDTree(ijk.astype(np.float64)).query_pairs(np.sqrt(link_r2) + 1e-6, output_type="ndarray")
    M = ijk.shape[0]
    graph = coo_matrix((np.ones(len(pairs)), (pairs[:, 0], pairs[:, 1])), shape=(M, M))
    _, labels = connected_components(graph, directed=False)
    _check_against_labels(ref, ijk, labels, f"{grid} r2={link_r2}")
    if grid in ("snake", "full"):
        assert ref["info"][1] == 1


@pytest.mark.parametrize("grid", list(GRIDS))
@pytest.mark.parametrize("link_r2,eps", [(1, 1.0), (4, 2.0)])
def test_restatement_matches_sklearn_dbscan(grid, link_r2, eps):
    cluster = pytest.importorskip("sklearn.cluster")
    occ = GRIDS[grid]()
    ref = OR.clusters(OR.grid_to_bits(occ[None]), RES, (0.25, -1.5, 3.0), 0.1, link_r2=link_r2)
    ijk = np.argwhere(occ)
    labels = cluster.DBSCAN(eps=eps, min_samples=1).fit_predict(ijk.astype(np.float64))
    assert labels.min() >= 0
    _check_against_labels(ref, ijk, labels, f"{grid} r2={link_r2}")


def test_restatement_options():
    occ = seeded_grid(0.08, 280)
    bits = OR.grid_to_bits(np.stack([np.zeros_like(occ), occ, occ]))
    full = OR.clusters(bits, RES, (0, 0, 0), 0.1, link_r2=3)
    np.testing.assert_array_equal(full["cluster_counts"], [0, full["info"][1] // 2, full["info"][1] // 2])
    K = int(full["info"][1])
    np.testing.assert_array_equal(full["rows"][:K // 2, 1:], full["rows"][K // 2:, 1:])          # two classes: independent, identical clusters
    big = OR.clusters(bits, RES, (0, 0, 0), 0.1, link_r2=3, min_cluster_voxels=3)
    assert 0 < big["info"][1] < K and (big["rows"][:, 1] >= 3).all() and (big["voxel_cluster"] == -1).any()
    kept = full["rows"][full["rows"][:, 1] >= 3]
    np.testing.assert_array_equal(big["rows"], kept)
    capped = OR.clusters(bits, RES, (0, 0, 0), 0.1, link_r2=3, max_clusters=2)
    assert capped["rows"].shape[0] == 2 and capped["info"].tolist() == [int(full["info"][0]), K, 0, 1]
    over = OR.clusters(bits, RES, (0, 0, 0), 0.1, link_r2=3, max_voxels=int(full["info"][0]) - 1)
    assert over["rows"] is None and over["info"].tolist() == [int(full["info"][0]), 0, 1, 0]
    np.testing.assert_array_equal(OR.counts(bits, RES), [0, occ.sum(), occ.sum()])


def test_float_centres_at_eps_02_lose_links():
    """The definition's reason: on the float64 voxel centres (i + 0.5) * 0.1, two voxels two apart along an axis are 0.2 or
    0.20000000000000004 apart depending on i, and DBSCAN(eps=0.2)'s `<= eps` links only some of the pairs that integer r2 = 4 links."""
    occ = seeded_grid(0.08, 280)
    ijk = np.argwhere(occ)
    d2 = ((ijk[:, None, :] - ijk[None, :, :]) ** 2).sum(-1)
    iu = np.triu_indices(len(ijk), 1)
    n_int = int((d2[iu] <= 4).sum())
    centres = (ijk.astype(np.float64) + 0.5) * 0.1
    dist = np.sqrt(((centres[:, None, :] - centres[None, :, :]) ** 2).sum(-1))
    n_float = int((dist[iu] <= 0.2).sum())
    lost = dist[iu][(d2[iu] <= 4) & ~(dist[iu] <= 0.2)]
    print(f"{len(ijk)} set voxels: {n_int} integer pairs with d2 <= 4, {n_float} float-centre pairs with dist <= 0.2; lost at {sorted(set(lost.tolist()))}")
    assert n_float < n_int
    assert ((dist[iu] <= 0.2) <= (d2[iu] <= 4)).all()               # float links are a subset: only links are lost, none invented
    assert (lost > 0.2).all() and (lost < 0.2 + 1e-15).all()


# ------------------------------------------------------------------ the match, hand-worked (every coordinate exactly representable)
MATCH_CASES = OR.MATCH_CASES


@pytest.mark.parametrize("case", list(MATCH_CASES))
def test_match_hand_worked(case):
    rows, locs, cls, thresh, want_det, want_match, want_gt = MATCH_CASES[case]
    det, mt, gm = OR.match(rows, 3, locs, cls, thresh)
    assert det.tolist() == want_det and mt.tolist() == want_match and gm.tolist() == want_gt


def test_insert_restatement_hand_worked():
    """Three pixels on a 4 x 4 x 4 grid of 0.5 m voxels at the origin: one inside, one exactly on the upper face (outside), one on a cell face
    (belongs to the upper cell)."""
    o = np.zeros((3, 3), np.float32)
    d = np.array([[1, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    keep, cls, ijk = OR.insert_voxels(o, d, [0.75, 2.0, 1.0], (0, 0, 0), 0.5, (4, 4, 4), 3, labels=[1, 1, 2])
    assert keep.tolist() == [True, False, True] and ijk[0].tolist() == [1, 0, 0] and ijk[2].tolist() == [0, 2, 0]
    bits = OR.pack_bits(cls[keep], ijk[keep], (4, 4, 4), 3)
    assert bits.shape == (3, 2) and bits[1, 0] == 1 << 16 and bits[2, 0] == 1 << 8 and bits[0].sum() == 0
