"""GPU tests of the semantic object map (csrc/objmap.hip, apnrf_amd/objects.py) against the numpy restatement tests/objmap_ref.py, which
tests/test_objmap_cpu.py holds against sklearn's DBSCAN and scipy's connected components.  Every comparison is `array_equal`: bit-grid
bytes, integers, and the float64 centroids bit for bit (integer sums, one float64 expression)."""
import ctypes

import numpy as np
import pytest
import torch

import helpers as H
import objmap_ref as OR
from objmap_ref import GRIDS, MATCH_CASES, RES, seeded_grid

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CANARY = 64


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


# ------------------------------------------------------------------ insert
G_RES, G_MIN, G_VS, G_C = (7, 5, 9), (0.5, 0.25, 1.0), 0.25, 5
MIN_DEPTH, MAX_DEPTH, MIN_ACC = 0.125, 4.0, 0.375


def _new_map(res=G_RES, gmin=G_MIN, vs=G_VS, C=G_C, first_class=1):
    from apnrf_amd.objects import SemanticObjectMap
    aabb = list(gmin) + [gmin[k] + res[k] * vs for k in range(3)]
    m = SemanticObjectMap(aabb, voxel_size=vs, num_classes=C, first_class=first_class, device=DEV)
    assert m.resolution == tuple(res) and m.words_per_plane == OR.words_per_plane(res)
    return m


def _insert_case(seed=0, N=4096, C=G_C):
    """Rays, depths, acc, logits and labels with every edge the insert has.  The first block of pixels is axis-aligned: o_k = 0, d = e_k, so that
    p_k = depth exactly, with depths one ulp below, on, and one ulp above every cell face of that axis (the six grid faces included)."""
    rng = np.random.default_rng(seed)
    f32 = np.float32
    lo, hi = np.array(G_MIN, f32), np.array(G_MIN, f32) + np.array(G_RES, f32) * f32(G_VS)
    o = rng.uniform(lo - 0.5, hi + 0.5, (N, 3)).astype(f32)
    d = rng.normal(size=(N, 3)).astype(f32)
    d /= np.linalg.norm(d, axis=1, keepdims=True).astype(f32)
    depth = rng.uniform(0.0, 2.5, N).astype(f32)
    n = 0
    for k in range(3):
        for i in range(G_RES[k] + 1):
            face = f32(G_MIN[k]) + f32(i) * f32(G_VS)
            for t in (np.nextafter(face, f32(-np.inf)), face, np.nextafter(face, f32(np.inf))):
                if n >= N:
                    break
                o[n] = (lo + hi) / 2                                 # the other two axes: mid-grid
                o[n, k] = 0.0
                d[n] = 0.0
                d[n, k] = 1.0
                depth[n] = t
                n += 1
    n_faces = n
    special = [np.nan, np.inf, -np.inf, 0.0, -1.0, MIN_DEPTH, MAX_DEPTH, np.nextafter(f32(MIN_DEPTH), f32(1)), np.nextafter(f32(MAX_DEPTH), f32(9))]
    if N >= n_faces + 4 * len(special):
        for j, s in enumerate(special * 4):
            depth[n_faces + j] = s
            o[n_faces + j] = (lo + hi) / 2                           # o + s d stays in the grid for the finite ones below ~0.8: the depth test decides
            d[n_faces + j] *= f32(0.05)
    acc = rng.uniform(0.0, 1.0, N).astype(f32)
    acc[::7] = MIN_ACC
    acc[3::7] = np.nextafter(f32(MIN_ACC), f32(0))
    acc[5::11] = np.nan
    sem = rng.normal(size=(N, C)).astype(f32)
    sem[::5, 1:4] = sem[::5, 1:2]                                    # ties between classes 1, 2, 3, often the maximum: the first wins
    sem[::9] = 0.25                                                  # all tied: class 0, never inserted at first_class 1
    sem[4::13, 2] = np.nan                                           # a NaN counts as the maximum
    labels = rng.integers(0, C, N).astype(np.int64)
    labels[::6] = 0
    labels[1::17] = C
    labels[2::19] = 255
    labels[3::23] = -1
    return dict(o=o, d=d, depth=depth, acc=acc, sem=sem, labels=labels, n_faces=n_faces)


def _ref_insert(case, route, C=G_C, sl=slice(None), bits=None, res=G_RES, gmin=G_MIN, vs=G_VS, **kw):
    if bits is None:
        bits = np.zeros((C, OR.words_per_plane(res)), np.uint32)
    src = dict(sem=case["sem"][sl]) if route == "sem" else dict(labels=_labels(case, route)[sl])
    return OR.insert(bits, case["o"][sl], case["d"][sl], case["depth"][sl], gmin, vs, res, acc=case["acc"][sl], min_depth=MIN_DEPTH,
                     max_depth=MAX_DEPTH, min_acc=MIN_ACC, **src, **kw)


def _labels(case, route):
    """u8 storage cannot hold -1: those pixels carry 255 there (also outside [0, C))."""
    lab = case["labels"]
    return np.where(lab < 0, 255, lab).astype(np.uint8) if route == "u8" else lab


def _gpu_insert(m, case, route, sl=slice(None)):
    src = dict(sem=_dev(case["sem"][sl])) if route == "sem" else dict(labels=_dev(_labels(case, route)[sl]))
    m.insert(_dev(case["o"][sl]), _dev(case["d"][sl]), _dev(case["depth"][sl]), acc=_dev(case["acc"][sl]), min_depth=MIN_DEPTH, max_depth=MAX_DEPTH,
             min_acc=MIN_ACC, **src)


@pytest.fixture(scope="module")
def case():
    return _insert_case()


@pytest.mark.parametrize("route", ["sem", "i64", "u8"])
def test_insert_bit_for_bit(case, route):
    m = _new_map()
    _gpu_insert(m, case, route)
    want = _ref_insert(case, route)
    np.testing.assert_array_equal(_u32(m.bits), want)
    np.testing.assert_array_equal(m.voxel_counts().cpu().numpy(), OR.counts(want, G_RES))
    assert want[0].sum() == 0 and all(want[c].any() for c in range(1, G_C))                      # class 0 never, every other class somewhere
    # the face pixels of the fixture do what the definition says: on a face -> the upper cell; one ulp outside a grid face -> dropped
    keep, _, ijk = OR.insert_voxels(case["o"], case["d"], case["depth"], G_MIN, G_VS, G_RES, G_C, first_class=0, labels=np.ones(len(case["depth"]), np.int64))
    n = 0
    for k in range(3):
        for i in range(G_RES[k] + 1):
            below, on, above = keep[n:n + 3], ijk[n:n + 3, k], None
            assert below[0] == (i > 0) and below[1] == (i < G_RES[k]) and below[2] == (i < G_RES[k]), (k, i, below)
            if i > 0:
                assert on[0] == i - 1
            if i < G_RES[k]:
                assert on[1] == i and on[2] == i
            n += 3
    assert n == case["n_faces"]


def test_insert_first_class_zero_and_no_acc(case):
    m = _new_map(first_class=0)
    m.insert(_dev(case["o"]), _dev(case["d"]), _dev(case["depth"]), sem=_dev(case["sem"]))
    want = OR.insert(np.zeros((G_C, OR.words_per_plane(G_RES)), np.uint32), case["o"], case["d"], case["depth"], G_MIN, G_VS, G_RES, first_class=0,
                     sem=case["sem"])
    np.testing.assert_array_equal(_u32(m.bits), want)
    assert want[0].any()


@pytest.mark.parametrize("N", [1000, 257, 1, 0])
def test_insert_29_classes_ragged_tiles(N):
    """C = 29 logits through the LDS staging with N that is no multiple of the tile (256 pixels at C = 29), one pixel, and none."""
    c = _insert_case(seed=N + 1, N=max(N, 1), C=29)
    m = _new_map(C=29)
    sl = slice(0, N)
    _gpu_insert(m, c, "sem", sl)
    want = _ref_insert(c, "sem", C=29, sl=sl)
    np.testing.assert_array_equal(_u32(m.bits), want)
    assert want.any() == (N >= 257)


@pytest.mark.parametrize("route", ["sem", "u8"])
def test_insert_accumulates(case, route):
    whole = _new_map()
    _gpu_insert(whole, case, route)
    halves = _new_map()
    _gpu_insert(halves, case, route, slice(0, 2048))
    first = _u32(halves.bits).copy()
    _gpu_insert(halves, case, route, slice(2048, 4096))
    np.testing.assert_array_equal(_u32(halves.bits), _u32(whole.bits))
    assert (first != _u32(whole.bits)).any()                                                     # the second half added something
    _gpu_insert(halves, case, route)                                                             # the same data again: nothing changes
    np.testing.assert_array_equal(_u32(halves.bits), _u32(whole.bits))
    halves.clear()
    assert not _u32(halves.bits).any()


# ------------------------------------------------------------------ clusters
def gpu_clusters(bits, res, gmin=(0.25, -1.5, 3.0), vs=0.1, link_r2=4, minv=1, max_voxels=None, max_clusters=None, exact_ws=False):
    """mnf_object_map_clusters through the C ABI on a uint32 [C, wpp] host grid, every output followed by a canary region and (unless `exact_ws`)
    the workspace too; returns host arrays and asserts the canaries."""
    from apnrf_amd import _lib as L
    lib = L.load_library()
    C = bits.shape[0]
    M = int(OR.counts(bits, res).sum())
    mv = M if max_voxels is None else max_voxels
    mc = mv if max_clusters is None else max_clusters
    b = _dev(bits.view(np.int32))
    out = dict(clusters=torch.full((mc * 5 + CANARY,), -777.0, dtype=torch.float64, device=DEV),
               cluster_counts=torch.full((C + CANARY,), -777, dtype=torch.int64, device=DEV), info=torch.full((4 + CANARY,), -777, dtype=torch.int64, device=DEV),
               voxel_ids=torch.full((mv + CANARY,), -777, dtype=torch.int64, device=DEV),
               voxel_cluster=torch.full((mv + CANARY,), -777, dtype=torch.int32, device=DEV))
    nbytes = int(lib.mnf_object_map_clusters_workspace_bytes(C, *res, mv))
    assert nbytes > 0 and nbytes % 8 == 0
    ws = torch.full((nbytes + (0 if exact_ws else 8 * CANARY),), 0xA5, dtype=torch.uint8, device=DEV)
    g = (ctypes.c_float * 3)(*gmin)
    L.launch(lib.mnf_object_map_clusters, L.ptr(b), C, *res, g, float(np.float32(vs)), link_r2, minv, mv, mc, L.ptr(out["clusters"]),
             L.ptr(out["cluster_counts"]), L.ptr(out["info"]), L.ptr(out["voxel_ids"]), L.ptr(out["voxel_cluster"]), L.ptr(ws), nbytes)
    torch.cuda.synchronize()
    host = {k: v.cpu().numpy() for k, v in out.items()}
    sizes = dict(clusters=mc * 5, cluster_counts=C, info=4, voxel_ids=mv, voxel_cluster=mv)
    for k, n in sizes.items():
        assert (host[k][n:] == -777).all(), f"{k}: written past its capacity"
        host[k] = host[k][:n]
    if not exact_ws:
        assert (ws[nbytes:].cpu().numpy() == 0xA5).all(), "written past the workspace"
    host["clusters"] = host["clusters"].reshape(mc, 5)
    host["raw"] = out
    return host


def _assert_clusters(got, ref, what=""):
    np.testing.assert_array_equal(got["info"], ref["info"], err_msg=what)
    K = ref["rows"].shape[0]
    np.testing.assert_array_equal(got["clusters"][:K].view(np.int64), ref["rows"].view(np.int64), err_msg=what)          # float64 bit patterns
    assert (got["clusters"][K:] == -777.0).all(), what                                                                    # rows beyond the found ones: untouched
    np.testing.assert_array_equal(got["cluster_counts"], ref["cluster_counts"], err_msg=what)
    M = int(ref["info"][0])
    np.testing.assert_array_equal(got["voxel_ids"][:M], ref["voxel_ids"], err_msg=what)
    np.testing.assert_array_equal(got["voxel_cluster"][:M], ref["voxel_cluster"], err_msg=what)
    assert (got["voxel_ids"][M:] == -777).all() and (got["voxel_cluster"][M:] == -777).all(), what


def _both(occ, link_r2=4, gmin=(0.25, -1.5, 3.0), vs=0.1, **kw):
    """occ bool [C,X,Y,Z] -> (gpu, ref)"""
    res = occ.shape[1:]
    bits = OR.grid_to_bits(occ)
    ref = OR.clusters(bits, res, gmin, vs, link_r2=link_r2, min_cluster_voxels=kw.get("minv", 1), max_voxels=kw.get("max_voxels"),
                      max_clusters=kw.get("max_clusters"))
    return gpu_clusters(bits, res, gmin, vs, link_r2, **kw), ref


@pytest.mark.parametrize("grid", ["fill8", "fill40", "snake", "full"])
def test_clusters_every_radius(grid):
    occ = GRIDS[grid]()[None]
    n = set()
    for r2 in range(1, 9):
        got, ref = _both(occ, r2)
        _assert_clusters(got, ref, f"{grid} r2={r2}")
        n.add(int(ref["info"][1]))
    if grid in ("snake", "full"):
        assert n == {1}
    else:
        assert len(n) > 1                                            # the radius matters on these grids


def test_clusters_many_workgroups():
    """64 x 16 x 64 at 5 %: ~3300 set voxels in 2048 words, a dozen workgroups of the link pass hooking into the same components."""
    occ = seeded_grid(0.05, 250, (64, 16, 64))[None]
    for r2 in range(1, 9):
        got, ref = _both(occ, r2)
        _assert_clusters(got, ref, f"r2={r2}")
    assert ref["info"][0] > 2560


def test_clusters_two_classes_are_independent():
    occ1 = seeded_grid(0.08, 280)
    occ = np.stack([occ1, np.zeros_like(occ1), occ1])
    got, ref = _both(occ, 4)
    _assert_clusters(got, ref)
    K = int(ref["info"][1]) // 2
    assert got["cluster_counts"].tolist() == [K, 0, K]
    np.testing.assert_array_equal(got["clusters"][:K, 1:], got["clusters"][K:2 * K, 1:])
    assert (got["clusters"][:K, 0] == 0).all() and (got["clusters"][K:2 * K, 0] == 2).all()


@pytest.mark.parametrize("offset,d2", [((2, 0, 0), 4), ((1, 1, 1), 3), ((2, 1, 0), 5), ((2, 2, 0), 8), ((0, 0, 1), 1), ((0, 2, 2), 8), ((1, 0, 2), 5)])
def test_pairs_link_exactly_as_link_r2_says(offset, d2):
    for sign in (1, -1):
        occ = np.zeros((1, 7, 7, 7), bool)
        a = np.array([3, 3, 3])
        b = a + sign * np.array(offset) * np.array([1, -1, 1])        # mixed signs along the axes
        occ[0, a[0], a[1], a[2]] = occ[0, b[0], b[1], b[2]] = True
        for r2 in range(1, 9):
            got, ref = _both(occ, r2)
            _assert_clusters(got, ref, f"{offset} r2={r2}")
            assert int(got["info"][1]) == (1 if d2 <= r2 else 2), (offset, r2)


def test_linear_neighbours_far_apart_in_space_do_not_link():
    X, Y, Z = 5, 4, 6
    a = np.zeros((1, X, Y, Z), bool)
    a[0, 2, 1, Z - 1] = a[0, 2, 2, 0] = True                         # linear indices differ by 1; (0, 1, -(Z-1)) apart
    b = np.zeros((1, X, Y, Z), bool)
    b[0, 2, Y - 1, Z - 1] = b[0, 3, 0, 0] = True                     # the same across an x step
    for occ in (a, b):
        for r2 in (1, 4, 8):
            got, ref = _both(occ, r2)
            _assert_clusters(got, ref)
            assert int(got["info"][1]) == 2


@pytest.mark.parametrize("res", [(4, 4, 4), (3, 3, 3), (7, 5, 9)])
def test_last_voxel_of_a_class_and_first_of_the_next_do_not_link(res):
    """Planes are adjacent in memory (64 voxels: no padding bit at all between the two)."""
    occ = np.zeros((3,) + res, bool)
    occ[1, -1, -1, -1] = occ[2, 0, 0, 0] = True
    occ[1, -2, -1, -1] = True                                        # ... while the last two of class 1 do link
    for r2 in (1, 8):
        got, ref = _both(occ, r2)
        _assert_clusters(got, ref)
        assert got["cluster_counts"].tolist() == [0, 1, 1] and got["clusters"][:2, 1].tolist() == [2.0, 1.0]


def test_padding_bits_are_ignored():
    """A caller that filled the tail of a plane: readers mask it."""
    res = (3, 3, 3)                                                  # 27 voxels in 2 words: 37 padding bits
    occ = np.zeros((2,) + res, bool)
    occ[0, 2, 2, 2] = occ[1, 0, 0, 0] = True
    bits = OR.grid_to_bits(occ)
    ref = OR.clusters(bits, res, (0, 0, 0), 0.5)
    dirty = bits.copy()
    dirty[:, 0] |= np.uint32(0xF8000000)
    dirty[:, 1] = 0xFFFFFFFF
    got = gpu_clusters(dirty, res, (0, 0, 0), 0.5, max_voxels=2)
    _assert_clusters(got, ref)
    from apnrf_amd import _lib as L
    cnt = torch.empty(2, dtype=torch.int64, device=DEV)
    d_bits = _dev(dirty.view(np.int32))
    L.launch(L.load_library().mnf_object_map_count, L.ptr(d_bits), 2, *res, L.ptr(cnt))
    assert cnt.tolist() == [1, 1]


def test_empty_grid_writes_nothing():
    got, ref = _both(np.zeros((2,) + RES, bool), 4, max_voxels=16, max_clusters=16)
    _assert_clusters(got, ref)
    assert got["info"].tolist() == [0, 0, 0, 0] and got["cluster_counts"].tolist() == [0, 0]
    got, ref = _both(np.zeros((2,) + RES, bool), 4)                  # ... and with no capacity at all
    assert got["info"].tolist() == [0, 0, 0, 0]


def test_min_cluster_voxels():
    occ = seeded_grid(0.08, 280)[None]
    got, ref = _both(occ, 3, minv=3)
    _assert_clusters(got, ref)
    assert (got["voxel_cluster"] == -1).any() and (got["clusters"][:int(ref["info"][1]), 1] >= 3).all() and ref["info"][1] > 0


def test_capacities():
    occ = np.zeros((2, 8, 8, 8), bool)
    for k in range(7):                                               # seven single-voxel clusters, four of class 0 and three of class 1
        occ[k % 2, k, (3 * k) % 8, 7 - k] = True
    occ[1, 5, 7, 3] = occ[1, 5, 7, 4] = True                         # ... and class 1's last, (5, 7, 2), gets company: 7 clusters, 9 voxels
    full, ref = _both(occ, 4, exact_ws=True)
    _assert_clusters(full, ref)
    assert full["info"].tolist() == [9, 7, 0, 0]
    got, ref = _both(occ, 4, max_voxels=8, exact_ws=True)            # one below the set count: only info
    assert got["info"].tolist() == [9, 0, 1, 0] == ref["info"].tolist()
    assert (got["clusters"] == -777.0).all() and (got["cluster_counts"] == -777).all() and (got["voxel_ids"] == -777).all()
    assert (got["voxel_cluster"] == -777).all()
    got, ref = _both(occ, 4, max_clusters=2, exact_ws=True)          # two of seven rows
    assert got["info"].tolist() == [9, 7, 0, 1]
    _assert_clusters(got, ref)
    np.testing.assert_array_equal(got["clusters"], full["clusters"][:2])
    np.testing.assert_array_equal(got["voxel_cluster"], full["voxel_cluster"])                   # true row numbers, also beyond the capacity
    got, ref = _both(occ, 4, max_voxels=20, max_clusters=20)         # spare capacity: the spare entries stay untouched
    _assert_clusters(got, ref)


def test_clusters_are_deterministic():
    occ = GRIDS["fill40"]()[None]
    runs = [gpu_clusters(OR.grid_to_bits(occ), RES, link_r2=4) for _ in range(3)]
    for r in runs[1:]:
        for k in ("clusters", "cluster_counts", "info", "voxel_ids", "voxel_cluster"):
            assert runs[0][k].tobytes() == r[k].tobytes(), k


# ------------------------------------------------------------------ match
def gpu_match(rows, C, locs, cls, thresh, max_clusters=None, info=None):
    from apnrf_amd import _lib as L
    lib = L.load_library()
    K = rows.shape[0]
    mc = K if max_clusters is None else max_clusters
    G = len(cls)
    buf = np.full((mc, 5), -777.0)
    buf[:K] = rows
    info = np.array([0, K, 0, 0], np.int64) if info is None else info
    detected = torch.full((C + CANARY,), -777, dtype=torch.int32, device=DEV)
    match = torch.full((mc + CANARY,), -777, dtype=torch.int32, device=DEV)
    gt_match = torch.full((G + CANARY,), -777, dtype=torch.int32, device=DEV)
    d_rows, d_info = _dev(buf), _dev(info)                           # named: they must outlive the launch
    d_locs, d_cls = _dev(np.asarray(locs, np.float64).reshape(-1, 3)), _dev(np.asarray(cls, np.int32))
    L.launch(lib.mnf_object_map_match, L.ptr(d_rows), L.ptr(d_info), mc, C, L.ptr(d_locs), L.ptr(d_cls), G, float(thresh), L.ptr(detected), L.ptr(match),
             L.ptr(gt_match))
    torch.cuda.synchronize()
    d, m, g = detected.cpu().numpy(), match.cpu().numpy(), gt_match.cpu().numpy()
    written = min(K, mc)
    assert (d[C:] == -777).all() and (m[written:] == -777).all() and (g[G:] == -777).all()
    return d[:C], m[:written], g[:G]


@pytest.mark.parametrize("case", list(MATCH_CASES))
def test_match_hand_worked(case):
    rows, locs, cls, thresh, want_det, want_match, want_gt = MATCH_CASES[case]
    det, mt, gm = gpu_match(rows, 3, locs, cls, thresh)
    assert det.tolist() == want_det and mt.tolist() == want_match and gm.tolist() == want_gt


@pytest.mark.parametrize("G,K,seed", [(200, 300, 1), (65, 40, 2), (7, 120, 3), (0, 12, 4), (30, 0, 5)])
def test_match_seeded(G, K, seed):
    """Clusters and objects on a 1/8 m lattice (plenty of exactly tied distances, and distances of exactly 1.0) across 28 classes, plus objects of
    classes the map does not have."""
    rng = np.random.default_rng(seed)
    C = 29
    rows = np.zeros((K, 5))
    rows[:, 0] = np.sort(rng.integers(1, C, K))
    rows[:, 1] = rng.integers(1, 50, K)
    rows[:, 2:] = rng.integers(-24, 25, (K, 3)) / 8.0
    cls = rng.integers(1, C, G).astype(np.int32)
    cls[::11] = rng.choice([-1, 0, C, 1000], len(cls[::11]))
    locs = rng.integers(-24, 25, (G, 3)) / 8.0
    for thresh in (1.0, 2.5, 100.0):
        want = OR.match(rows, C, locs, cls, thresh)
        got = gpu_match(rows, C, locs, cls, thresh, max_clusters=K + 5)
        for a, b in zip(got, want):
            np.testing.assert_array_equal(a, b)
    if G == 200:
        assert 0 < want[0].sum() < min(G, K) and (want[1] >= 0).sum() == want[0].sum() == (want[2] >= 0).sum()


def test_match_after_voxel_overflow_finds_nothing():
    rows, locs, cls, thresh = MATCH_CASES["tie"][:4]
    det, mt, gm = gpu_match(rows[:0], 3, locs, cls, thresh, max_clusters=4, info=np.array([9, 0, 1, 0], np.int64))
    assert det.tolist() == [0, 0, 0] and gm.tolist() == [-1, -1]


# ------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def scene():
    return H.make_scene(log2_hashmap_size=15)


@pytest.fixture(scope="module")
def model(scene):
    return H.hip_field(scene), H.hip_estimator(scene)


def _objects(res_rows, rng, C):
    """A made-up ground-truth list: some objects near cluster centroids (detectable), some far, some of classes without clusters."""
    locs, cls = [], []
    for k in range(0, res_rows.shape[0], 3):
        locs.append(res_rows[k, 2:] + rng.integers(-3, 4, 3) / 4.0)
        cls.append(int(res_rows[k, 0]))
    for _ in range(10):
        locs.append(rng.uniform(-30, 30, 3))
        cls.append(int(rng.integers(0, C)))
    return np.array(locs, np.float64).reshape(-1, 3), np.array(cls, np.int32)


def _assert_detect(m, want_bits, seed):
    ref = OR.clusters(want_bits, m.resolution, m.grid_min, m.voxel_size, link_r2=4)
    locs, cls = _objects(ref["rows"], np.random.default_rng(seed), m.num_classes)
    got = m.detect(locs, cls, det_dist_thresh=1.0, points=True)
    det, mt, gm = OR.match(ref["rows"], m.num_classes, locs, cls, 1.0)
    np.testing.assert_array_equal(got["detected"], det)
    np.testing.assert_array_equal(got["match"], mt)
    np.testing.assert_array_equal(got["gt_match"], gm)
    assert got["total"] == int(det.sum())
    np.testing.assert_array_equal(got["class"], ref["rows"][:, 0].astype(np.int64))
    np.testing.assert_array_equal(got["count"], ref["rows"][:, 1].astype(np.int64))
    np.testing.assert_array_equal(got["centroid"].view(np.int64), ref["rows"][:, 2:].copy().view(np.int64))
    np.testing.assert_array_equal(got["per_class"], ref["cluster_counts"])
    np.testing.assert_array_equal(got["point_cluster"], ref["voxel_cluster"])
    n = int(np.prod(m.resolution))
    np.testing.assert_array_equal(got["point_class"], ref["voxel_ids"] // n)
    np.testing.assert_array_equal(got["point_voxel"], OR.unravel(ref["voxel_ids"] % n, m.resolution))
    plain = m.clusters(link_r2=4)
    np.testing.assert_array_equal(plain["centroid"], got["centroid"])
    return got


def test_insert_views_end_to_end(scene, model):
    """The map of 4 rendered poses (320 x 320 at scale 0.1: 32 x 32 rays each) equals the restatement's insert of the same planes, rendered
    separately through `render_views` and copied to the host; `detect` equals the restatement's clusters and match."""
    from apnrf_amd import render as RD
    from apnrf_amd.objects import SemanticObjectMap
    field, est = model
    kw = H.RENDER_KW
    poses = scene["poses"][:4]
    width = height = 320
    focal = 0.5 * width / np.tan(np.pi / 4)
    m = SemanticObjectMap(scene["aabb"], voxel_size=0.2, num_classes=29, device=DEV)
    ins = dict(min_depth=0.05, max_depth=8.0, min_acc=0.5)
    m.insert_views(field, est, poses, width, height, focal, kw["near_plane"], kw["render_step_size"], 0.1, kw["cone_angle"], kw["alpha_thre"], **ins)
    o, d, h, w = RD._pose_rays(np.asarray(poses), width, height, focal, 0.1, DEV)
    assert (h, w) == (32, 32)
    r = RD.render_views(field, est, o, d, h * w, 1024, near_plane=kw["near_plane"], render_step_size=kw["render_step_size"], render_bkgd=torch.zeros(3),
                        cone_angle=kw["cone_angle"], alpha_thre=kw["alpha_thre"], image_hw=(h, w), n_split=None)
    want = OR.insert(np.zeros((29, m.words_per_plane), np.uint32), o.cpu().numpy(), d.cpu().numpy(), r["depth"].cpu().numpy().reshape(-1), m.grid_min,
                     m.voxel_size, m.resolution, sem=r["sem"].cpu().numpy().reshape(-1, 29), acc=r["acc"].cpu().numpy().reshape(-1), **ins)
    np.testing.assert_array_equal(_u32(m.bits), want)
    counts = OR.counts(want, m.resolution)
    assert counts[0] == 0 and counts.sum() > 100 and (counts > 0).sum() > 1                      # not an empty map, more than one class
    got = _assert_detect(m, want, 7)
    assert got["total"] > 0


@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("depth_along", ["z", "ray"])
def test_insert_dataset_end_to_end(scene, tmp_path, packed, depth_along):
    from apnrf_amd import render as RD
    from apnrf_amd.dataset import Dataset
    from apnrf_amd.objects import SemanticObjectMap, planar_to_ray_scale
    rng = np.random.default_rng(11)
    n_img, h, w, C = 3, 24, 20, 29
    c2w = np.stack([RD.pose_to_c2w(np.asarray(p, np.float64)) for p in scene["poses"][:n_img]]).astype(np.float32)
    depths = rng.uniform(0.3, 6.0, (n_img, h, w)).astype(np.float32)
    depths[:, ::5, ::3] = 0.0                                        # Habitat's "no return"
    sems = rng.integers(0, C, (n_img, h, w)).astype(np.int64)
    ds = Dataset(training=False, save_fp=str(tmp_path / "ds"), device=DEV, packed=packed)
    ds.update_data(rng.integers(0, 256, (n_img, h, w, 3), dtype=np.uint8), depths, sems, c2w)
    assert ds.semantics.dtype == (torch.uint8 if packed else torch.int64)
    ids = [2, 0]
    m = SemanticObjectMap(scene["aabb"], voxel_size=0.2, num_classes=C, device=DEV)
    m.insert_dataset(ds, ids, depth_along=depth_along)
    rays = RD.generate_image_rays(c2w[ids], w, h, ds.K, DEV)
    stored = ds.depths[ids].to(torch.float32).cpu().numpy().reshape(len(ids), -1)                # what the storage holds (fp16-rounded when packed)
    if depth_along == "z":
        scale = planar_to_ray_scale(w, h, float(ds.K[0, 0]), DEV).cpu().numpy()
        f = float(ds.K[0, 0])
        x, y = np.meshgrid((np.arange(w) - w / 2 + 0.5) / f, (np.arange(h) - h / 2 + 0.5) / f)
        np.testing.assert_allclose(scale, np.sqrt(x * x + y * y + 1.0).reshape(-1), rtol=1e-6)  # |cam| of the pixel, row-major
        stored = stored * scale[None]                                # one float32 multiplication, as torch does it
    want = OR.insert(np.zeros((C, m.words_per_plane), np.uint32), rays.origins.cpu().numpy(), rays.viewdirs.cpu().numpy(), stored.reshape(-1), m.grid_min,
                     m.voxel_size, m.resolution, labels=sems[ids].reshape(-1))
    np.testing.assert_array_equal(_u32(m.bits), want)
    assert OR.counts(want, m.resolution)[1:].sum() > 200 and OR.counts(want, m.resolution)[0] == 0
    _assert_detect(m, want, 13)
