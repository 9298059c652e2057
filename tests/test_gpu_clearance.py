"""GPU tests of the trajectory-clearance unit (csrc/clearance.hip, apnrf_amd/clearance.py) against the numpy restatement
tests/clearance_ref.py, which tests/test_clearance_cpu.py holds to the reference's own answers (tests/golden/clearance_walks.npz) and to
scipy.  Every integer comparison is `array_equal`; outputs of the C ABI are allocated with canaries on both sides.  The float64 values the
Python module forms with torch are compared with numpy's same expressions within 8 ulp of the largest operand: each is at most six
rounded operations and one square root, every one of them within half an ulp of a value no larger than the largest operand (the device's
square root is not assumed to be numpy's bit for bit, only correctly rounded to within one ulp)."""
import ctypes
import types

import numpy as np
import pytest
import torch

import clearance_ref as CR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CANARY = 64
MARK32, MARK64 = -0x5A5A5A5B, -0x5A5A5A5A5A5A5A5B


def _dev(a):
    return torch.from_numpy(np.array(a, copy=True, order="C")).to(DEV)


def _guarded(n, dtype, mark):
    whole = torch.full((n + 2 * CANARY,), mark, dtype=dtype, device=DEV)
    return whole, whole[CANARY:CANARY + n]


def _assert_guards(whole, n, mark, what):
    host = whole.cpu().numpy()
    assert (host[:CANARY] == mark).all() and (host[CANARY + n:] == mark).all(), f"{what}: written outside its bounds"


def _lib():
    from apnrf_amd import _lib as L
    return L, L.load_library()


# ------------------------------------------------------------------ the field
def gpu_field(binaries):
    """mnf_clearance_field through the C ABI, twice -> (d2 [X,Y,Z] int32, info [2]) on the host; the second call must give the same bytes."""
    L, lib = _lib()
    b = np.ascontiguousarray(binaries, np.uint8)
    M, X, Y, Z = b.shape
    d_b = _dev(b)
    outs = []
    for _ in range(2):
        dw, d2 = _guarded(X * Y * Z, torch.int32, MARK32)
        iw, info = _guarded(2, torch.int64, MARK64)
        L.launch(lib.mnf_clearance_field, L.ptr(d_b), M, X, Y, Z, L.ptr(d2), L.ptr(info), device=torch.device(DEV))
        torch.cuda.synchronize()
        _assert_guards(dw, X * Y * Z, MARK32, "d2")
        _assert_guards(iw, 2, MARK64, "info")
        outs.append((d2.cpu().numpy().reshape(X, Y, Z), info.cpu().numpy()))
    assert outs[0][0].tobytes() == outs[1][0].tobytes() and outs[0][1].tobytes() == outs[1][1].tobytes()
    return outs[0]


def _sparse(shape, seed, p, members=1):
    rng = np.random.default_rng(seed)
    return (rng.uniform(size=(members,) + tuple(shape)) < p).astype(np.uint8)


def _one(shape, at, members=1, member=0):
    g = np.zeros((members,) + tuple(shape), np.uint8)
    g[(member,) + tuple(at)] = 1
    return g


def _full_but_one(shape, at):
    g = np.ones((1,) + tuple(shape), np.uint8)
    g[(0,) + tuple(at)] = 0
    return g


def _empty_lines_and_planes():
    g = np.zeros((1, 20, 12, 70), np.uint8)
    g[0, 3, 2:5, 10:60:7] = 1                                    # one plane of x holds everything: 19 empty planes, and empty lines within it
    g[0, 3, 9, 69] = 3                                           # any non-zero byte counts
    return g


# name -> the members' grids.  Beyond the issue's list: the sizes at which the passes take another path (an axis of one voxel has no
# pass; with Z = 1 the lines along y lie back to back; 64, 32, 16 or 8 columns per tile as the axis grows; a line of 2048).
FIELD_CASES = {
    "13x9x70": lambda: _sparse((13, 9, 70), 1, 0.02, members=2),
    "67x130x5": lambda: _sparse((67, 130, 5), 2, 0.004),
    "empty": lambda: np.zeros((2, 5, 6, 7), np.uint8),
    "corner": lambda: _one((7, 5, 9), (6, 4, 8)),
    "full_but_one": lambda: _full_but_one((6, 7, 5), (2, 3, 1)),
    "empty_lines_and_planes": _empty_lines_and_planes,
    "member_1_only": lambda: _one((5, 4, 6), (1, 2, 3), members=2, member=1),
    "1x1x1": lambda: np.ones((1, 1, 1, 1), np.uint8),
    "1x1x1_empty": lambda: np.zeros((1, 1, 1, 1), np.uint8),
    "z_of_one": lambda: _sparse((9, 70, 1), 3, 0.02),
    "x_only": lambda: _sparse((300, 1, 1), 4, 0.01),
    "x_of_one": lambda: _sparse((1, 40, 33), 5, 0.01),
    "32_columns": lambda: _sparse((300, 3, 5), 6, 0.003),
    "16_columns": lambda: _sparse((2, 600, 3), 7, 0.003),
    "8_columns": lambda: _one((2048, 2, 5), (2047, 1, 4)),
    "line_of_2048": lambda: _one((3, 2, 2048), (0, 1, 2047)),
}
_REF = {}


def field_case(name):
    """(grids, brute-force d2, info): computed once per session and shared, read-only."""
    if name not in _REF:
        g = FIELD_CASES[name]()
        d2, info = CR.brute_d2(g)
        for a in (g, d2, info):
            a.setflags(write=False)
        _REF[name] = (g, d2, info)
    return _REF[name]


@pytest.mark.parametrize("name", list(FIELD_CASES))
def test_field_equals_brute_force(name):
    g, want, want_info = field_case(name)
    got, info = gpu_field(g)
    np.testing.assert_array_equal(got, want, err_msg=name)
    np.testing.assert_array_equal(info, want_info, err_msg=name + " info")
    if name in ("empty", "1x1x1_empty"):
        assert (got == CR.INT32_MAX).all() and info.tolist() == [0, -1]
    if name == "8_columns":
        assert got[0, 0, 0] == 2047 * 2047 + 1 + 16                                    # the largest distance an axis of 2048 gives, plus the others


def test_field_refuses_geometry_without_a_launch():
    L, lib = _lib()
    d_b, d_o, d_i = _dev(np.zeros(8, np.uint8)), torch.zeros(8, dtype=torch.int32, device=DEV), torch.zeros(2, dtype=torch.int64, device=DEV)
    for shape in ((2049, 1, 1), (1, 2049, 1), (1, 1, 2049), (0, 1, 1), (2048, 2048, 2048)):
        with pytest.raises(L.MnfError):
            L.launch(lib.mnf_clearance_field, L.ptr(d_b), 1, *shape, L.ptr(d_o), L.ptr(d_i), device=torch.device(DEV))
    with pytest.raises(L.MnfError):
        L.launch(lib.mnf_clearance_field, L.ptr(d_b), 0, 2, 2, 2, L.ptr(d_o), L.ptr(d_i), device=torch.device(DEV))
    torch.cuda.synchronize()
    assert int(d_o.abs().sum()) == 0 and d_i.tolist() == [0, 0]


# ------------------------------------------------------------------ the lookup
ORIGIN = np.array([-0.6, 0.4, -0.2])
VOXEL = 0.2


def gpu_lookup(d2, origin, voxel, points, offsets):
    L, lib = _lib()
    d2 = np.ascontiguousarray(d2, np.int32)
    X, Y, Z = d2.shape
    p = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
    off = np.ascontiguousarray(offsets, np.int64)
    P, T = p.shape[0], off.shape[0] - 1
    cw, cells = _guarded(3 * P, torch.int32, MARK32)
    pw, pd2 = _guarded(P, torch.int32, MARK32)
    tw, traj = _guarded(4 * T, torch.int64, MARK64)
    iw, info = _guarded(2, torch.int64, MARK64)
    info.zero_()
    d_d2, d_p, d_off = _dev(d2), _dev(p), _dev(off)
    L.launch(lib.mnf_clearance_lookup, L.ptr(d_d2), X, Y, Z, (ctypes.c_double * 3)(*[float(v) for v in origin]), float(voxel), L.ptr(d_p) if P else None, P,
             L.ptr(d_off), T, L.ptr(cells) if P else None, L.ptr(pd2) if P else None, L.ptr(traj) if T else None, L.ptr(info), device=torch.device(DEV))
    torch.cuda.synchronize()
    for w, n, m, what in ((cw, 3 * P, MARK32, "cells"), (pw, P, MARK32, "point_d2"), (tw, 4 * T, MARK64, "traj"), (iw, 2, MARK64, "info")):
        _assert_guards(w, n, m, what)
    return cells.cpu().numpy().reshape(P, 3), pd2.cpu().numpy(), traj.cpu().numpy().reshape(T, 4), info.cpu().numpy()


def lookup_inputs():
    """Trajectories over the 13 x 9 x 70 grid: an empty one, a single sample, 300 samples inside (more than one workgroup's turn), one with
    samples outside and samples that are not finite, one whose minimum is attained twice, one wholly outside."""
    rng = np.random.default_rng(17)
    ext = np.array([13, 9, 70]) * VOXEL
    inside = lambda n: ORIGIN + rng.uniform(0.02, 0.98, (n, 3)) * ext
    mixed = inside(40)
    mixed[3] = ORIGIN - 0.05
    mixed[7, 1] = ORIGIN[1] + ext[1] + 0.01
    mixed[11, 0] = np.nan
    mixed[12, 2] = np.inf
    mixed[13] = -np.inf
    mixed[14, 0] = 1e300
    tie = inside(30)
    tie[20] = tie[4] + [0.0, 0.0, 1e-3]                          # most likely the same voxel: the same d2 again, later
    out = ORIGIN + ext + rng.uniform(0.1, 3.0, (5, 3))
    parts = [np.zeros((0, 3)), inside(1), inside(300), mixed, tie, out]
    offsets = np.concatenate([[0], np.cumsum([len(q) for q in parts])]).astype(np.int64)
    return np.concatenate(parts), offsets


def test_lookup_equals_the_restatement():
    _, d2, _ = field_case("13x9x70")
    pts, offsets = lookup_inputs()
    want = CR.lookup(d2, ORIGIN, VOXEL, pts, offsets)
    got = gpu_lookup(d2, ORIGIN, VOXEL, pts, offsets)
    for g, w, what in zip(got, want, ("cells", "point_d2", "traj", "info")):
        np.testing.assert_array_equal(g, w, err_msg=what)
    traj = want[2]
    assert traj[0].tolist() == [-1, -1, 0, 0] and traj[1, 3] == 1 and traj[3, 2] >= 6 and traj[5].tolist() == [-1, -1, 5, 5]
    assert want[3].tolist()[1] == 3                                                    # three samples are not finite


def test_lookup_ties_resolve_to_the_first_sample():
    g, d2, _ = field_case("corner")                                                    # 7 x 5 x 9, one voxel at (6, 4, 8)
    centre = lambda c: (np.array(c) + 0.5) * VOXEL
    pts = np.array([centre((0, 0, 0)), centre((5, 4, 6)), centre((6, 2, 7)), centre((4, 4, 8)), centre((6, 4, 6))])   # d2 116, 5, 5, 4, 4
    rev = pts[::-1].copy()
    offsets = [0, 5, 10, 13]
    allp = np.concatenate([pts, rev, pts[:3]])
    want = CR.lookup(d2, [0, 0, 0], VOXEL, allp, offsets)
    assert want[1][:5].tolist() == [116, 5, 5, 4, 4]
    assert want[2].tolist() == [[4, 3, 0, 5], [4, 0, 0, 5], [5, 1, 0, 3]]
    got = gpu_lookup(d2, [0, 0, 0], VOXEL, allp, offsets)
    for a, b in zip(got, want):
        np.testing.assert_array_equal(a, b)


def test_lookup_pinned_values_give_the_reference_cells(golden):
    w = golden("clearance_walks")
    pinned, cells = w["pinned"], w["pinned_cells"]
    d2 = np.zeros((41, 2, 2), np.int32)
    pts = np.stack([pinned, np.full_like(pinned, 0.1), np.full_like(pinned, 0.3)], axis=1)
    got = gpu_lookup(d2, [0.0, 0.0, 0.0], float(w["size"]), pts, [0, pts.shape[0]])
    np.testing.assert_array_equal(got[0][:, 0], cells)
    assert (got[0][:, 1] == 0).all() and (got[0][:, 2] == 1).all()
    assert (cells != np.floor(pinned / float(w["size"]))).any() and got[0][5, 0] == 4                  # 1.0 // 0.2
    assert got[2][0].tolist() == [0, 0, int((cells < 0).sum() + (cells > 40).sum()), pts.shape[0]]


def test_lookup_decimal_values_and_the_neighbours_of_faces():
    """The values a planner hands over are decimals (3.0 // 0.2 is 14), and the doubles next to a face k * 0.2 on either side."""
    faces = np.arange(41) * 0.2
    vals = np.concatenate([np.arange(400) / 10.0, np.arange(400) / 100.0, np.nextafter(faces, 100.0), np.nextafter(faces, -100.0), -np.arange(1, 60) / 10.0])
    with np.errstate(invalid="ignore"):
        want = (vals // 0.2).astype(np.int64)
    assert want[30] == 14 and (want != np.floor(vals / 0.2)).any()
    pts = np.stack([np.full_like(vals, 0.1), vals, np.full_like(vals, 0.1)], axis=1)
    got = gpu_lookup(np.zeros((2, 3, 2), np.int32), [0.0, 0.0, 0.0], 0.2, pts, [0, vals.shape[0]])
    np.testing.assert_array_equal(got[0][:, 1], want)


def test_lookup_no_trajectories_is_a_no_op_and_bad_offsets_touch_nothing():
    _, d2, _ = field_case("corner")
    got = gpu_lookup(d2, [0, 0, 0], VOXEL, np.zeros((0, 3)), [0])
    assert got[3].tolist() == [0, 0]
    pts = np.full((4, 3), 0.1)
    got = gpu_lookup(d2, [0, 0, 0], VOXEL, pts, [-7, 2, 900])                         # clamped to [0, 4]: the canaries are checked
    assert got[2][:, 3].tolist() == [2, 2]


# ------------------------------------------------------------------ the walks
def gpu_walk_count(start, end, cur, endv, size, max_steps):
    L, lib = _lib()
    n = len(start)
    cw, counts = _guarded(n, torch.int64, MARK64)
    iw, info = _guarded(3, torch.int64, MARK64)
    info.zero_()
    d = [_dev(np.asarray(start, np.float64)), _dev(np.asarray(end, np.float64)), _dev(np.asarray(cur, np.int32)), _dev(np.asarray(endv, np.int32))]
    L.launch(lib.mnf_voxel_walk_count, *[L.ptr(t) for t in d], n, float(size), int(max_steps), L.ptr(counts), L.ptr(info), device=torch.device(DEV))
    torch.cuda.synchronize()
    _assert_guards(cw, n, MARK64, "counts")
    _assert_guards(iw, 3, MARK64, "info")
    return counts.cpu().numpy(), info.cpu().numpy()


def gpu_walk_fill(start, end, cur, endv, size, max_steps, offsets, total):
    L, lib = _lib()
    n = len(start)
    vw, vox = _guarded(3 * total, torch.int32, MARK32)
    iw, info = _guarded(3, torch.int64, MARK64)
    info.zero_()
    d = [_dev(np.asarray(start, np.float64)), _dev(np.asarray(end, np.float64)), _dev(np.asarray(cur, np.int32)), _dev(np.asarray(endv, np.int32))]
    d_off = _dev(np.asarray(offsets, np.int64))
    L.launch(lib.mnf_voxel_walk_fill, *[L.ptr(t) for t in d], n, float(size), int(max_steps), L.ptr(d_off), total, L.ptr(vox) if total else None, L.ptr(info),
             device=torch.device(DEV))
    torch.cuda.synchronize()
    _assert_guards(vw, 3 * total, MARK32, "voxels")
    _assert_guards(iw, 3, MARK64, "info")
    return vox.cpu().numpy().reshape(total, 3), info.cpu().numpy()


def gpu_walk_hits(start, end, cur, endv, size, max_steps, grids):
    L, lib = _lib()
    n = len(start)
    g = np.ascontiguousarray(grids, np.uint8)
    M, X, Y, Z = g.shape
    hw, hits = _guarded(5 * n, torch.int32, MARK32)
    iw, info = _guarded(3, torch.int64, MARK64)
    info.zero_()
    d = [_dev(np.asarray(start, np.float64)), _dev(np.asarray(end, np.float64)), _dev(np.asarray(cur, np.int32)), _dev(np.asarray(endv, np.int32))]
    d_g = _dev(g)
    L.launch(lib.mnf_voxel_walk_hits, *[L.ptr(t) for t in d], n, float(size), int(max_steps), L.ptr(d_g), M, X, Y, Z, L.ptr(hits), L.ptr(info),
             device=torch.device(DEV))
    torch.cuda.synchronize()
    _assert_guards(hw, 5 * n, MARK32, "hits")
    _assert_guards(iw, 3, MARK64, "info")
    return hits.cpu().numpy().reshape(n, 5), info.cpu().numpy()


@pytest.fixture(scope="module")
def walks(golden):
    g = golden("clearance_walks")
    return {k: g[k] for k in g.files}


def test_walk_counts_and_lists_equal_the_reference(walks):
    args = (walks["start"], walks["end"], walks["current_voxel"], walks["end_voxel"], float(walks["size"]), 4096)
    counts, info = gpu_walk_count(*args)
    np.testing.assert_array_equal(counts, np.diff(walks["offsets"]))
    assert info.tolist() == [0, 0, 0]
    vox, info = gpu_walk_fill(*args, walks["offsets"], int(walks["offsets"][-1]))
    np.testing.assert_array_equal(vox, walks["voxels"])
    assert info.tolist() == [0, 0, 0]


def test_walk_hit_rows_equal_the_reference_lists(walks):
    args = (walks["start"], walks["end"], walks["current_voxel"], walks["end_voxel"], float(walks["size"]), 4096)
    off = walks["offsets"]
    lists = [walks["voxels"][off[i]:off[i + 1]] for i in range(len(off) - 1)]
    for grids in (walks["grid"], walks["grid"][:1], walks["grid"][1:]):
        want = np.stack([CR.walk_hit(v, grids) for v in lists])
        got, info = gpu_walk_hits(*args, grids)
        np.testing.assert_array_equal(got, want)
        assert info.tolist() == [0, 0, 0]
    np.testing.assert_array_equal(want_member0_bools(lists, walks["grid"]), walks["checker"])      # what the reference's checker answered


def want_member0_bools(lists, grid):
    return np.array([CR.walk_hit(v, grid[:1])[0] >= 0 for v in lists])


def test_collision_checker_gives_the_reference_bools(walks, capsys):
    from apnrf_amd import clearance as C
    size, shape = float(walks["size"]), walks["shape"]
    grid = _dev(walks["grid"])
    got = []
    for i in range(walks["start"].shape[0]):
        aabb = np.concatenate([walks["origin"][i], walks["origin"][i] + shape * size])
        x = np.stack([walks["start"][i], 0.5 * (walks["start"][i] + walks["end"][i]), walks["end"][i]])
        r = C.collision_checker(grid, {"x": x}, size, aabb)
        assert isinstance(r, bool)
        got.append(r)
    np.testing.assert_array_equal(np.array(got), walks["checker"])
    assert C.collision_checker(walks["grid"], {"x": x}, size, aabb) == got[-1]          # a host grid goes up by itself
    assert capsys.readouterr().out == ""                                              # and nothing is printed


def test_voxels_between_points_is_the_reference_list(walks):
    from apnrf_amd import clearance as C
    off = walks["offsets"]
    for i in (0, 90, int(np.flatnonzero(walks["kind"] == 5)[0]), int(np.flatnonzero(walks["kind"] == 2)[0]), len(off) - 2):
        got = C.voxels_between_points(walks["start"][i], walks["end"][i], walks["current_voxel"][i], walks["end_voxel"][i], float(walks["size"]))
        assert isinstance(got, list) and all(v.shape == (3,) and v.dtype == np.int32 for v in got)
        np.testing.assert_array_equal(np.array(got).reshape(-1, 3), walks["voxels"][off[i]:off[i + 1]])
    with pytest.raises(C.L.MnfError):                                                  # a cut walk would not be the reference's list
        C.voxels_between_points([0.1, 0.1, 0.1], [5.1, 3.1, 0.1], np.array([0, 0, 0]), np.array([25, 15, 0]), 0.2, max_steps=7)


def test_cut_and_non_finite_walks_are_counted_and_stay_in_their_rows():
    start = np.array([[0.1, 0.1, 0.1], [0.1, np.nan, 0.1], [0.5, 0.5, 0.5], [0.1, 0.1, 0.1], [np.inf, 0.1, 0.1]])
    end = np.array([[5.1, 3.1, 0.1], [5.1, 3.1, 0.1], [0.7, 0.5, 0.5], [0.1, 0.1, -np.inf], [0.3, 0.1, 0.1]])
    cur = np.array([[0, 0, 0], [0, 0, 0], [2, 2, 2], [0, 0, 0], [0, 0, 0]], np.int32)
    endv = np.array([[25, 15, 0], [25, 15, 0], [3, 2, 2], [0, 0, -5], [1, 0, 0]], np.int32)
    ref = [CR.voxel_walk(start[i], end[i], cur[i], endv[i], 0.2, max_steps=7) for i in range(5)]
    assert [r[1] for r in ref] == [True, False, False, False, False] and [r[2] for r in ref] == [True, False, True, False, False]
    counts, info = gpu_walk_count(start, end, cur, endv, 0.2, 7)
    assert counts.tolist() == [len(r[0]) for r in ref] == [7, 0, 2, 0, 0] and info.tolist() == [1, 3, 0]
    offsets = np.concatenate([[0], np.cumsum(counts)])
    vox, info = gpu_walk_fill(start, end, cur, endv, 0.2, 7, offsets, int(offsets[-1]))
    np.testing.assert_array_equal(vox, np.concatenate([r[0] for r in ref]))
    assert info.tolist() == [1, 3, 0]
    grid = np.zeros((1, 30, 20, 4), np.uint8)
    grid[0, 3, 2, 0] = 1
    hits, info = gpu_walk_hits(start, end, cur, endv, 0.2, 7, grid)
    np.testing.assert_array_equal(hits, np.stack([CR.walk_hit(r[0], grid) for r in ref]))
    assert info.tolist() == [1, 3, 0] and hits[0, 0] >= 0 and hits[0, 4] == 7
    # slots that are not the walks' lengths: nothing leaves a slot, every mismatch is counted
    short = np.array([0, 3, 3, 4, 4, 4], np.int64)
    vox, info = gpu_walk_fill(start, end, cur, endv, 0.2, 7, short, 4)
    np.testing.assert_array_equal(vox[:3], ref[0][0][:3])
    np.testing.assert_array_equal(vox[3], ref[2][0][0])
    assert info.tolist() == [1, 3, 2]
    wild = np.array([0, 900, -5, 2, 2, 2], np.int64)                                  # slots outside [0, total): skipped and counted
    vox, info = gpu_walk_fill(start, end, cur, endv, 0.2, 7, wild, 4)
    assert (vox == MARK32).all() and info[2] == 3
    # max_steps 0 lists nothing
    counts, info = gpu_walk_count(start[:1], end[:1], cur[:1], endv[:1], 0.2, 0)
    assert counts.tolist() == [0] and info.tolist() == [1, 0, 0]


def test_walk_argument_errors_and_empty_batch():
    L, lib = _lib()
    info = torch.zeros(3, dtype=torch.int64, device=DEV)
    L.launch(lib.mnf_voxel_walk_count, None, None, None, None, 0, 0.2, 10, None, L.ptr(info), device=torch.device(DEV))
    d = [torch.zeros(3, dtype=torch.float64, device=DEV), torch.zeros(3, dtype=torch.float64, device=DEV), torch.zeros(3, dtype=torch.int32, device=DEV),
         torch.zeros(3, dtype=torch.int32, device=DEV)]
    counts = torch.zeros(1, dtype=torch.int64, device=DEV)
    for size, steps in ((0.0, 10), (-0.2, 10), (float("nan"), 10), (float("inf"), 10), (0.2, -1), (0.2, 1 << 31)):
        with pytest.raises(L.MnfError):
            L.launch(lib.mnf_voxel_walk_count, *[L.ptr(t) for t in d], 1, size, steps, L.ptr(counts), L.ptr(info), device=torch.device(DEV))
    torch.cuda.synchronize()
    assert info.tolist() == [0, 0, 0]


# ------------------------------------------------------------------ the Python module
def _ulp_close(got, want, operand, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, what
    both_nan = np.isnan(got) & np.isnan(want)
    same_inf = np.isinf(want) & (got == want)
    tol = 8 * np.spacing(np.maximum(np.abs(np.broadcast_to(operand, want.shape)), np.abs(np.where(np.isfinite(want), want, 0.0))))
    with np.errstate(invalid="ignore"):
        ok = both_nan | same_inf | (np.abs(got - want) <= tol)
    assert ok.all(), f"{what}: {np.flatnonzero(~ok)[:5]} beyond 8 ulp"


def test_module_field_from_estimators_and_arrays():
    from apnrf_amd import clearance as C
    g, want, want_info = field_case("13x9x70")
    aabb = np.concatenate([ORIGIN, ORIGIN + np.array(g.shape[1:]) * VOXEL])
    ests = [types.SimpleNamespace(binaries=_dev(np.stack([g[m], np.ones_like(g[m])]).astype(bool)), aabbs=_dev(np.stack([aabb, aabb * 2]).astype(np.float32)))
            for m in range(2)]                                                         # level 1 is full: only level 0 may be read
    f = C.clearance_field(ests)
    np.testing.assert_array_equal(f.d2.cpu().numpy(), want)
    np.testing.assert_array_equal(f.info.cpu().numpy(), want_info)
    assert f.d2.is_cuda and f.aabb.is_cuda and f.voxel.is_cuda and f.info.is_cuda and abs(float(f.voxel) - VOXEL) < 1e-6
    f2 = C.clearance_field(g, aabb=aabb, device=DEV)
    assert torch.equal(f2.d2, f.d2) and float(f2.voxel) == float(np.float64((aabb[3] - aabb[0]) / 13))
    with pytest.raises(ValueError):
        C.clearance_field(g, aabb=[0, 0, 0, 1, 1, 1], device=DEV)                      # not cubic
    with pytest.raises(ValueError):
        C.clearance_field(g, aabb=aabb, voxel=0.25, device=DEV)                        # not this grid's edge
    with pytest.raises(C.L.MnfError):
        C.clearance_field(np.zeros((1, 2049, 1, 1), np.uint8), aabb=[0, 0, 0, 2049, 1, 1], device=DEV)


def test_module_trajectory_clearance_values():
    from apnrf_amd import clearance as C
    g, d2, _ = field_case("13x9x70")
    aabb = np.concatenate([ORIGIN, ORIGIN + np.array(g.shape[1:]) * VOXEL])
    f = C.clearance_field(g, aabb=aabb, device=DEV)
    voxel = float(f.voxel)
    pts, offsets = lookup_inputs()
    radius = 0.05
    out = f.trajectory_clearance(pts, offsets, radius=radius, host=True)
    assert all(torch.is_tensor(out[k]) and out[k].is_cuda for k in ("cells", "point_d2", "traj", "metres", "lower", "margin", "certified", "closest"))
    cells, pd2, traj, info = CR.lookup(d2, ORIGIN, voxel, pts, offsets)
    np.testing.assert_array_equal(out["cells"].cpu().numpy(), cells)
    np.testing.assert_array_equal(out["point_d2"].cpu().numpy(), pd2)
    np.testing.assert_array_equal(out["traj"].cpu().numpy(), traj)
    np.testing.assert_array_equal(out["summary"]["traj"], traj)
    inside = pd2 >= 0
    root = np.sqrt(np.maximum(pd2, 0).astype(np.float64))
    metres = np.where(inside, root * voxel, np.nan)
    lower = np.where(inside, np.maximum(root - CR.SQRT3, 0.0) * voxel, 0.0)
    _ulp_close(out["metres"].cpu().numpy(), metres, np.maximum(root, voxel), "metres")
    _ulp_close(out["lower"].cpu().numpy(), lower, np.maximum(root, CR.SQRT3), "lower")
    P, T = pts.shape[0], offsets.shape[0] - 1
    tid = np.searchsorted(offsets[1:], np.arange(P), side="right")
    margin = np.full(P, np.inf)
    operand = np.ones(P)
    with np.errstate(invalid="ignore", over="ignore"):
        d = pts[1:] - pts[:-1]
        length = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        seg = ((lower[:-1] + lower[1:]) - length) / 2
    same = tid[:-1] == tid[1:]
    margin[:-1][same] = seg[same]
    with np.errstate(invalid="ignore"):
        big = np.nanmax(np.abs(np.where(np.isfinite(pts), pts, 0.0)), axis=1)
    operand[:-1] = np.maximum.reduce([big[:-1], big[1:], np.where(np.isfinite(length), length, 0.0), lower[:-1], lower[1:]])
    single = (np.diff(offsets) == 1)[np.minimum(tid, T - 1)] & (tid < T)
    margin[single] = lower[single]
    _ulp_close(out["margin"].cpu().numpy(), margin, operand, "margin")
    # the verdict, as the numbers say; no margin sits within rounding of the radius
    finite = np.isfinite(margin)
    assert (np.abs(margin[finite] - radius) > 1e-9).all()
    with np.errstate(invalid="ignore"):
        ok = margin > radius
    want_cert = np.array([bool(ok[offsets[t]:offsets[t + 1]].all()) and traj[t, 2] == 0 for t in range(T)])
    np.testing.assert_array_equal(out["certified"].cpu().numpy(), want_cert)
    np.testing.assert_array_equal(out["summary"]["certified"], want_cert)
    assert want_cert[0] and not want_cert[3] and not want_cert[5]                       # empty: vacuous; samples outside: never
    closest = np.where(traj[:, 0] >= 0, np.sqrt(np.maximum(traj[:, 0], 0).astype(np.float64)) * voxel, np.nan)
    _ulp_close(out["closest"].cpu().numpy(), closest, np.sqrt(np.maximum(traj[:, 0], 1).astype(np.float64)), "closest")
    # sample_traj's x, z, y order is the same trajectory with two columns swapped
    swapped = f.trajectory_clearance(pts[:, [0, 2, 1]], offsets, planner_axes=True, radius=radius)
    assert torch.equal(swapped["point_d2"], out["point_d2"]) and torch.equal(swapped["traj"], out["traj"])


def _gap_world():
    """A wall across x = 10 .. 11 with a gap of 9 voxels in z at heights 2 .. 10; 24 x 12 x 30 voxels of 0.2 m."""
    g = np.zeros((1, 24, 12, 30), np.uint8)
    g[0, 10:12, :, :] = 1
    g[0, 10:12, 2:11, 11:20] = 0
    return g, np.array([0.0, 0.0, 0.0, 4.8, 2.4, 6.0])


def test_module_planner_map_and_a_trajectory_through_a_gap():
    from apnrf_amd import clearance as C
    from apnrf_amd import planning as PL
    g, aabb = _gap_world()
    f = C.clearance_field(g, aabb=aabb, voxel=0.2, device=DEV)
    d2, _ = CR.brute_d2(g)
    np.testing.assert_array_equal(f.d2.cpu().numpy(), d2)
    for radius in (0.0, 0.3, 0.9):
        thr = C.d2_threshold(radius, 0.2)
        assert thr == CR.d2_threshold(radius, 0.2)
        m = f.planner_map(5, 8, thr)
        assert m.dtype == torch.int32 and m.is_cuda and tuple(m.shape) == (24, 30)
        np.testing.assert_array_equal(m.cpu().numpy(), (d2[:, 5:8, :] <= thr).any(axis=1).astype(np.int32))
    with pytest.raises(ValueError):
        f.planner_map(5, 5, 3)
    # the gap is open for a 0.3 m vehicle and closed for a 0.9 m one, and the grid search takes the map as it stands
    reach = {}
    for radius in (0.3, 0.9):
        field = PL.path_field(f.planner_map(5, 8, C.d2_threshold(radius, 0.2)), [[2, 15]])["field"][0].cpu().numpy()
        reach[radius] = field[20, 15] != -1
    assert reach[0.3] and not reach[0.9]
    # a straight flight through the middle of the gap, 5 cm between samples; and one that clips the wall
    t = np.linspace(0.0, 1.0, 65)[:, None]
    through = np.array([0.5, 1.3, 3.1]) + t * np.array([3.2, 0.0, 0.0])
    clipping = np.array([0.5, 1.3, 3.1]) + t * np.array([3.2, 0.0, 2.4])
    pts = np.concatenate([through, clipping])
    offsets = np.array([0, 65, 130])
    _, pd2, traj, _ = CR.lookup(d2, aabb[:3], 0.2, pts, offsets)
    lower = np.maximum(np.sqrt(pd2.astype(np.float64)) - CR.SQRT3, 0.0) * 0.2
    want = {}
    for radius in (0.2, 0.7):
        rows = []
        for a, b in ((0, 65), (65, 130)):
            seg = ((lower[a:b - 1] + lower[a + 1:b]) - np.linalg.norm(pts[a + 1:b] - pts[a:b - 1], axis=1)) / 2
            assert (np.abs(seg - radius) > 1e-9).all()
            rows.append(bool((seg > radius).all()))
        want[radius] = rows
    assert want[0.2] == [True, False] and want[0.7] == [False, False] and (traj[:, 2] == 0).all()
    for radius in (0.2, 0.7):
        out = f.trajectory_clearance(pts, offsets, radius=radius)
        assert out["certified"].cpu().tolist() == want[radius]
    assert out["traj"].cpu().numpy()[1, 0] == 0                                        # the clipping flight enters an occupied voxel


def test_module_sweep_equals_the_restatement():
    from apnrf_amd import clearance as C
    g, aabb = _gap_world()
    g = np.concatenate([g, np.zeros_like(g)])
    g[1, 20, 7, 16] = 1                                                                # member 1 holds one voxel beyond the gap, on the third segment's walk
    f = C.clearance_field(g, aabb=aabb, voxel=0.2, device=DEV)
    rng = np.random.default_rng(5)
    way = np.array([[0.5, 1.3, 3.1], [1.7, 1.3, 3.0], [2.9, 1.5, 3.3], [4.5, 1.3, 3.1], [4.5, 1.3, 0.5], [0.7, 0.5, 0.4]])
    other = rng.uniform([0.1, 0.1, 0.1], [4.7, 2.3, 5.9], (7, 3))
    other[3, 1] = np.nan
    pts = np.concatenate([way, other, way[:1]])
    offsets = np.array([0, 6, 13, 14])
    for members in (None, [0], [1]):
        out = f.sweep(pts, offsets, members=members, max_steps=64)
        grids = g if members is None else g[members]
        rel = pts - aabb[:3]
        cells = CR.cells_of_points(pts, aabb[:3], 0.2)
        want = np.full((14, 5), -1, np.int32)
        want[:, 4] = 0
        seg = np.zeros(14, bool)
        cut = bad = 0
        for t in range(3):
            for i in range(offsets[t], offsets[t + 1] - 1):
                v, c, fin = CR.voxel_walk(rel[i], rel[i + 1], cells[i], cells[i + 1], 0.2, max_steps=64)
                want[i] = CR.walk_hit(v, grids)
                seg[i] = True
                cut += c
                bad += not fin
        np.testing.assert_array_equal(out["hits"].cpu().numpy(), want)
        np.testing.assert_array_equal(out["segment"].cpu().numpy(), seg)
        assert out["info"].cpu().tolist() == [cut, bad, 0] and bad == 2
    assert want[2].tolist() == [5, 20, 7, 16, 9] and (want[[0, 1, 3, 4], 0] == -1).all()   # member 1 alone: its voxel is met, the wall is not there
