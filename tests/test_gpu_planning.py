"""GPU tests of the planner grid search (csrc/planning.hip, apnrf_amd/planning.py) against the numpy restatement tests/planning_ref.py,
which tests/test_planning_cpu.py holds to the reference's own answers (tests/golden/planner_paths.npz).  Every comparison is
`array_equal`: labels, cells, offsets and the bits of float64 positions.  Outputs of the C ABI are allocated with canaries on both
sides."""
import math
import os

import numpy as np
import pytest
import torch

import planning_ref as PR

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "planner_paths.npz")

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CANARY = 64
MARK32, MARK64 = -0x5A5A5A5B, -0x5A5A5A5A5A5A5A5B
CASES = ("small", "cut", "blocked_start", "rooms")


def _dev(a):
    return torch.from_numpy(np.array(a, copy=True, order="C")).to(DEV)


def case_of(g, name):
    return {k[len(name) + 1:]: g[k] for k in g.files if k.startswith(name + "_")}


@pytest.fixture(scope="module")
def fixture(golden):
    g = golden("planner_paths")
    return {name: case_of(g, name) for name in CASES}


def _guarded(n, dtype, mark):
    """A device buffer of n elements with CANARY marked elements on both sides -> (whole, middle view)."""
    whole = torch.full((n + 2 * CANARY,), mark, dtype=dtype, device=DEV)
    return whole, whole[CANARY:CANARY + n]


def _assert_guards(whole, n, mark, what):
    host = whole.cpu().numpy()
    assert (host[:CANARY] == mark).all() and (host[CANARY + n:] == mark).all(), f"{what}: written outside its bounds"


def gpu_fields(blocked, sources, limits=None):
    """mnf_path_field through the C ABI -> (uint32 [B,nx,ny], int64 [B,2]) on the host."""
    from apnrf_amd import _lib as L
    lib = L.load_library()
    blocked = np.asarray(blocked, np.int32)
    sources = np.asarray(sources, np.int32).reshape(-1, 2)
    nx, ny = blocked.shape[-2:]
    B = sources.shape[0]
    n_maps = 1 if blocked.ndim == 2 else blocked.shape[0]
    lim = (nx, ny) if limits is None else limits
    assert lib.mnf_path_field_bytes(nx, ny, B) == B * nx * ny * 4
    fw, field = _guarded(B * nx * ny, torch.int32, MARK32)
    iw, info = _guarded(2 * B, torch.int64, MARK64)
    d_map, d_src = _dev(blocked), _dev(sources)
    L.launch(lib.mnf_path_field, L.ptr(d_map), n_maps, nx, ny, lim[0], lim[1], L.ptr(d_src) if B else None, B, L.ptr(field) if B else None,
             L.ptr(info) if B else None, device=torch.device(DEV))
    torch.cuda.synchronize()
    _assert_guards(fw, B * nx * ny, MARK32, "field")
    _assert_guards(iw, 2 * B, MARK64, "info")
    return field.cpu().numpy().view(np.uint32).reshape(B, nx, ny), info.cpu().numpy().reshape(B, 2)


def gpu_trace(fields, goals, offsets, total):
    """mnf_path_trace through the C ABI on host arrays -> (paths [total,2] as left by the call, info [2])."""
    from apnrf_amd import _lib as L
    fields = np.asarray(fields, np.uint32)
    B, nx, ny = fields.shape
    goals = np.asarray(goals, np.int32).reshape(-1, 3)
    G = goals.shape[0]
    pw, paths = _guarded(2 * total, torch.int32, MARK32)
    iw, info = _guarded(2, torch.int64, MARK64)
    d_f, d_g, d_o = _dev(fields.view(np.int32)), _dev(goals), _dev(np.asarray(offsets, np.int64))
    L.launch(L.load_library().mnf_path_trace, L.ptr(d_f), B, nx, ny, L.ptr(d_g) if G else None, L.ptr(d_o), G, L.ptr(paths) if total else None,
             L.ptr(info), device=torch.device(DEV))
    torch.cuda.synchronize()
    _assert_guards(pw, 2 * total, MARK32, "paths")
    _assert_guards(iw, 2, MARK64, "info")
    return paths.cpu().numpy().reshape(total, 2), info.cpu().numpy()


def _assert_fields(blocked, sources, limits=None, what=""):
    got, info = gpu_fields(blocked, sources, limits)
    want, reached = PR.path_fields(blocked, sources, limits)
    np.testing.assert_array_equal(got, want, err_msg=what)
    np.testing.assert_array_equal(info[:, 0], reached, err_msg=what + " reached")
    nx, ny = np.asarray(blocked).shape[-2:]
    src = np.asarray(sources).reshape(-1, 2)
    inside = (src[:, 0] >= 0) & (src[:, 0] < nx) & (src[:, 1] >= 0) & (src[:, 1] < ny)
    assert ((info[:, 1] > 0) == inside).all() and (info[:, 1] <= nx * ny).all(), what
    return got, info


_SMALL = {}


def small_map():
    if "m" not in _SMALL:
        m = np.load(GOLDEN)["small_map"]                             # the fixture's 24 x 20 map
        m.setflags(write=False)
        _SMALL["m"] = m
    return _SMALL["m"]


# ------------------------------------------------------------------ fields, bit for bit
@pytest.mark.parametrize("shape,source", [((1, 1), (0, 0)), ((1, 7), (0, 2)), ((7, 1), (6, 0))])
def test_degenerate_maps(shape, source):
    got, info = _assert_fields(np.zeros(shape, np.int32), [source], what=str(shape))
    assert info[0, 0] == shape[0] * shape[1]
    if shape == (1, 1):
        assert got.tolist() == [[[0]]] and info[0].tolist() == [1, 1]
    blocked = np.zeros(shape, np.int32)
    blocked[-1, -1] = 1
    _assert_fields(blocked, [source, (0, 0)], what=f"{shape} with an obstacle")


def test_fixture_map_from_several_starts(fixture):
    m = fixture["small"]["map"]
    np.testing.assert_array_equal(m, small_map())
    starts = [tuple(fixture["small"]["start_cell"]), tuple(fixture["blocked_start"]["start_cell"]), (0, 0), (23, 19), (17, 6), (23, 0)]
    got, info = _assert_fields(m, starts, what="24 x 20")
    assert m[17, 6] == 0 and 0 < info[4, 0] < 40 and info[0, 0] > 250                      # inside the walled pocket / outside it
    # the reference's own answers: None flags and make-up of every goal
    c = fixture["small"]
    lab = got[0].reshape(-1)
    np.testing.assert_array_equal(lab == 0xFFFFFFFF, c["none"][:480])
    np.testing.assert_array_equal((lab >> 16)[~c["none"][:480]], c["ab"][:480, 0][~c["none"][:480]])
    np.testing.assert_array_equal((lab & 0xFFFF)[~c["none"][:480]], c["ab"][:480, 1][~c["none"][:480]])


def test_sizes_off_the_wave_and_the_banks():
    blocked = PR.seeded_map((65, 63), 11, 0.25)
    _assert_fields(blocked, [(32, 31), (0, 0), (64, 62)], what="65 x 63")


def test_serpentine_at_the_cap():
    """198 x 198, walls on every odd row open at alternating ends: the most sweeps a map of this size asks for, `a` near 19 600: both
    16-bit halves of the label and the sweep counter are exercised."""
    n = 198
    blocked = PR.serpentine(n)
    got, info = gpu_fields(blocked, [(0, 0)])
    want, reached = PR.path_field(blocked, (0, 0))
    np.testing.assert_array_equal(got[0], want)
    a, b, ok = PR.split(got[0])
    assert info[0, 0] == reached == (blocked == 0).sum() and ok[n - 2, 0]
    assert a[ok].max() > 19000 and b[ok].max() >= 98 and (a + b)[ok].max() == 19503
    assert 0 < info[0, 1] <= n * n                                                             # in-place updates may settle several moves per sweep


def test_fully_blocked_and_fully_free():
    got, info = _assert_fields(np.ones((31, 17), np.int32), [(15, 8)], what="blocked")
    assert info[0].tolist() == [1, 1] and got[0, 15, 8] == 0 and (got != 0).sum() == 31 * 17 - 1
    n, sx, sy = 198, 60, 131
    got, info = gpu_fields(np.zeros((n, n), np.int32), [(sx, sy)])
    dx, dy = np.abs(np.arange(n) - sx)[:, None], np.abs(np.arange(n) - sy)[None, :]
    want = ((np.abs(dx - dy) << 16) | np.minimum(dx, dy)).astype(np.uint32)                    # the closed form (|dx - dy|, min(dx, dy))
    np.testing.assert_array_equal(got[0], want)
    assert info[0, 0] == n * n and 0 < info[0, 1] <= n * n
    small, _ = _assert_fields(np.zeros((9, 14), np.int32), [(2, 11)], what="free")             # the restatement agrees with the closed form
    assert small[0, 8, 0] == (5 << 16) | 6


# ------------------------------------------------------------------ batching
@pytest.mark.parametrize("B", [1, 3, 300])
def test_one_map_many_sources(B):
    m = small_map()
    rng = np.random.default_rng(B)
    src = np.stack([rng.integers(0, 24, B), rng.integers(0, 20, B)], axis=1)
    got, info = _assert_fields(m, src, what=f"B = {B}")
    if B == 300:
        assert (m[src[:, 0], src[:, 1]] != 0).sum() > 50                                       # blocked sources among them


@pytest.mark.parametrize("B", [3, 300])
def test_one_map_per_source(B):
    shape = (12, 10) if B == 300 else (24, 20)
    maps = np.stack([PR.seeded_map(shape, 100 + i, 0.3) for i in range(B)])
    rng = np.random.default_rng(B + 1)
    src = np.stack([rng.integers(0, shape[0], B), rng.integers(0, shape[1], B)], axis=1)
    got, _ = _assert_fields(maps, src, what=f"{B} maps")
    assert len({g.tobytes() for g in got}) > B // 2


def test_sources_outside_the_map():
    m = small_map()
    src = [(3, 4), (24, 4), (-1, 0), (3, 20), (0, -1), (1 << 20, 5), (3, 4)]
    got, info = _assert_fields(m, src, what="outside")
    for b in (1, 2, 3, 4, 5):
        assert (got[b] == 0xFFFFFFFF).all() and info[b].tolist() == [0, 0]
    np.testing.assert_array_equal(got[0], got[6])
    empty, info = gpu_fields(m, np.zeros((0, 2), np.int32))                                    # n_sources = 0: a no-op
    assert empty.shape == (0, 24, 20) and info.shape == (0, 2)


def test_limits(fixture):
    c = fixture["cut"]
    lim = PR.limits_of(c["aabb"].tolist(), c["map"].shape, float(c["res"]))
    assert lim == (22, 20)
    got, _ = _assert_fields(c["map"], [c["start_cell"], (23, 5)], lim, what="cut")
    assert (got[0, 22:] == 0xFFFFFFFF).all() and (c["map"][22:] == 0).any()
    np.testing.assert_array_equal(got[0].reshape(-1) == 0xFFFFFFFF, c["none"])
    assert got[1, 23, 5] == 0 and (got[1] != 0xFFFFFFFF).sum() == 1                            # a source beyond the limits is left nowhere
    _assert_fields(c["map"], [c["start_cell"]], (24, 7), what="cut in y")
    _assert_fields(c["map"], [c["start_cell"]], (0, 0), what="no legal cell")


# ------------------------------------------------------------------ traces
@pytest.fixture(scope="module")
def small_field():
    m = small_map()
    fields, _ = PR.path_fields(m, [(3, 4), (17, 6)])
    fields.setflags(write=False)
    return fields


def test_trace_every_goal_in_one_launch(small_field):
    goals = np.array([[0, x, y] for x in range(24) for y in range(20)] + [[1, 17, 7], [1, 3, 4], [0, 24, 0], [0, 0, -1], [2, 3, 4], [-1, 3, 4]], np.int32)
    paths, offsets, lengths = PR.trace_many(small_field, goals)
    got, info = gpu_trace(small_field, goals, offsets, int(offsets[-1]))
    np.testing.assert_array_equal(got, paths)
    assert info.tolist() == [int((lengths > 0).sum()), 0]
    assert (lengths == 0).sum() > 100 and lengths.max() > 20 and lengths[-6] > 0 and (lengths[-5:] == 0).all()
    # the module: lengths and offsets formed on the device
    from apnrf_amd.planning import trace_paths
    t = trace_paths(_dev(small_field.view(np.int32)), _dev(goals))
    np.testing.assert_array_equal(t["paths"].cpu().numpy(), paths)
    np.testing.assert_array_equal(t["offsets"].cpu().numpy(), offsets)
    np.testing.assert_array_equal(t["lengths"].cpu().numpy(), lengths)
    assert t["paths"].dtype == torch.int32 and t["offsets"].dtype == torch.int64 and t["info"].cpu().tolist() == info.tolist()


def test_trace_of_no_goal(small_field):
    got, info = gpu_trace(small_field, np.zeros((0, 3), np.int32), [0], 0)
    assert got.shape == (0, 2) and info.tolist() == [0, 0]
    from apnrf_amd.planning import trace_paths
    t = trace_paths(_dev(small_field.view(np.int32)), torch.zeros(0, 3, dtype=torch.int32, device=DEV))
    assert t["paths"].shape == (0, 2) and t["offsets"].cpu().tolist() == [0] and t["lengths"].shape == (0,)


def test_trace_slots_that_do_not_fit(small_field):
    goals = np.array([[0, 10, 12], [0, 17, 6], [0, 3, 4], [0, 20, 18], [0, 4, 5]], np.int32)
    paths, offsets, lengths = PR.trace_many(small_field, goals)
    assert lengths[0] > 3 and lengths[1] == 0 and lengths[2] == 1 and lengths[3] > 3
    bad = offsets.copy()
    bad[1:] += 1                                                                               # goal 0: one cell too many
    bad[2:] += 1                                                                               # goal 1: a slot for an unreached goal
    bad[4:] -= 1                                                                               # goal 3: one cell too few
    total = int(bad[-1]) + 3
    got, info = gpu_trace(small_field, goals, bad, total)
    assert info.tolist() == [2, 3]
    want = np.full((total, 2), MARK32, np.int32)
    want[bad[2]:bad[3]] = paths[offsets[2]:offsets[3]]                                         # the two goals that fit are written, nothing else
    want[bad[4]:bad[5]] = paths[offsets[4]:offsets[5]]
    np.testing.assert_array_equal(got, want)


# ------------------------------------------------------------------ the reference's class
@pytest.mark.parametrize("name", CASES)
def test_dijkstra_against_the_reference(fixture, name):
    from apnrf_amd.planning import Dijkstra
    c = fixture[name]
    res = float(c["res"])
    d = Dijkstra(c["aabb"].tolist(), c["map"] if name != "rooms" else _dev(c["map"]), res, 0.05, device=DEV)
    lim = PR.limits_of(c["aabb"].tolist(), c["map"].shape, res)
    assert (d.lim_x, d.lim_y) == lim and (d.x_width, d.y_width) == c["map"].shape and d.min_x == 0 and d.resolution == res
    assert d.max_x == c["aabb"][3] - c["aabb"][0] and d.max_y == c["aabb"][4] - c["aabb"][1] and len(d.motion) == 8
    sx, sy = (float(v) for v in c["start"])
    field, _ = PR.path_field(c["map"], c["start_cell"], lim)
    got = d.planning_many(sx, sy, [tuple(g) for g in c["goals"].tolist()])
    assert d.fields_computed == 1
    assert [r is None for r in got] == c["none"].tolist()                                      # None on exactly the reference's goals
    for g, r in enumerate(got):
        if r is None:
            continue
        rx, ry = r
        assert isinstance(rx, list) and isinstance(ry, list) and len(rx) == len(ry) == c["len"][g]
        cells = PR.trace(field, c["goal_cells"][g])
        assert rx == [int(i) * res + 0 for i in cells[:, 0]] and ry == [int(i) * res + 0 for i in cells[:, 1]]      # bit-equal floats
        assert PR.make_up(cells) == tuple(c["ab"][g].tolist())
        assert (rx[0], ry[0]) == (c["goal_cells"][g, 0] * res, c["goal_cells"][g, 1] * res) and (rx[-1], ry[-1]) == (sx, sy)
    # one goal at a time: the cached field serves it
    some = [g for g in range(len(got)) if got[g] is not None][::37] + [int(np.nonzero(c["none"])[0][0])]
    for g in some:
        assert d.planning(sx, sy, *c["goals"][g].tolist()) == got[g]
    assert d.fields_computed == 1 and len(d._fields) == 1
    np.testing.assert_array_equal(d.reachable(sx, sy).cpu().numpy(), field != PR.UNREACHED)
    np.testing.assert_array_equal(d.costs(sx, sy).cpu().numpy(), PR.field_costs(field))
    assert d.fields_computed == 1
    other = np.argwhere(c["map"] == 0)[-1]
    assert d.planning(other[0] * res, other[1] * res, other[0] * res, other[1] * res) == ([other[0] * res], [other[1] * res])
    assert d.fields_computed == 2
    # a start outside the map: None for every goal, nothing launched
    assert d.planning_many(-5.0, 0.0, [(0.0, 0.0), (sx, sy)]) == [None, None] and d.planning(1000.0, 0.0, sx, sy) is None
    assert not d.reachable(-5.0, 0.0).any() and np.isinf(d.costs(-5.0, 0.0).cpu().numpy()).all() and d.fields_computed == 2


def test_module_functions(fixture):
    from apnrf_amd.planning import field_costs, path_field
    m = fixture["small"]["map"]
    src = [(3, 4), (17, 6), (30, 0)]
    out = path_field(_dev(m), src)
    want, reached = PR.path_fields(m, src)
    assert out["field"].dtype == torch.int32 and tuple(out["field"].shape) == (3, 24, 20) and out["info"].dtype == torch.int64
    np.testing.assert_array_equal(out["field"].cpu().numpy().view(np.uint32), want)
    np.testing.assert_array_equal(out["info"][:, 0].cpu().numpy(), reached)
    costs = field_costs(out["field"])
    assert costs.dtype == torch.float64
    np.testing.assert_array_equal(costs.cpu().numpy(), PR.field_costs(want))
    assert np.isinf(costs[2].cpu().numpy()).all() and costs[0, 3, 4] == 0.0 and costs[0, 4, 5].item() == math.sqrt(2.0)
    lim = path_field(_dev(m.astype(np.int64) * 7), [(3, 4)], limits=(22, 20))                  # any integer map: non-zero is blocked
    np.testing.assert_array_equal(lim["field"][0].cpu().numpy().view(np.uint32), PR.path_field(m, (3, 4), (22, 20))[0])
    from apnrf_amd import _lib as L
    with pytest.raises(L.MnfError):
        path_field(torch.zeros(199, 199, dtype=torch.int32, device=DEV), [(0, 0)])


# ------------------------------------------------------------------ chaining
def test_planner_map_feeds_the_field():
    """mnf_planner_map's device output of a two-member ensemble goes into path_field as it stands: no host copy in between."""
    from apnrf_amd import _lib as L
    from apnrf_amd.nerfacc import OccGridEstimator
    from apnrf_amd.planning import path_field
    from oracle import occgrid as OG
    res = (20, 12, 18)
    rng = np.random.default_rng(4)
    ests = []
    for _ in range(2):
        e = OccGridEstimator(torch.tensor([0.0, 0.0, 0.0, 4.0, 2.4, 3.6]), resolution=list(res), levels=1).to(DEV)
        e.binaries = torch.from_numpy(rng.random((1, *res)) > 0.985).to(DEV)
        ests.append(e)
    b = torch.stack([e.binaries[0] for e in ests]).contiguous().view(torch.uint8)
    planner_map = torch.empty(res[0], res[2], dtype=torch.int32, device=DEV)
    L.launch(L.load_library().mnf_planner_map, L.ptr(b), 2, *res, 8, L.ptr(planner_map))
    src = [(0, 0), (10, 9), (19, 17)]
    out = path_field(planner_map, src)
    ref_map = OG.planner_path_finding_map([e.binaries.cpu().numpy() for e in ests])
    np.testing.assert_array_equal(planner_map.cpu().numpy(), ref_map)
    assert 0.05 < ref_map.mean() < 0.8
    want, reached = PR.path_fields(ref_map, src)
    np.testing.assert_array_equal(out["field"].cpu().numpy().view(np.uint32), want)
    np.testing.assert_array_equal(out["info"][:, 0].cpu().numpy(), reached)
    assert reached.max() > 50


def test_exploration_map_goal_paths():
    """A hand-made 12 x 8 x 10 map: free floor, a wall across it with one gap, a walled-off corner, the rest unknown."""
    import explore_ref as ER
    from apnrf_amd.explore import ExplorationMap
    X, Y, Z = 12, 8, 10
    st = np.full((X, Y, Z), -1, np.int8)
    st[:, 2, :] = 0                                                  # free at layer 2
    st[6, 2, :] = 1                                                  # a wall across x = 6 ...
    st[6, 2, 7] = 0                                                  # ... with a gap
    st[9:, 2, 5] = 1                                                 # a closed corner: x >= 9, z <= 5
    st[9, 2, :6] = 1
    st[0, 2, 9] = -1                                                 # one unknown cell
    vs = 0.25
    m = ExplorationMap([1.0, 0.0, -2.0, 1.0 + X * vs, Y * vs, -2.0 + Z * vs], voxel_size=vs, max_range=5.0, device=DEV)
    assert m.resolution == (X, Y, Z)
    m.bits.copy_(_dev(ER.states_to_bits(st).view(np.int32)))
    current = (1.0 + 2.6 * vs, -2.0 + 1.4 * vs)                      # cell_of -> (2.1, 0.9): the cell (2, 1)
    goals = np.array([[11, 9], [11, 2], [2, 1], [0, 9], [6, 3], [12, 0]], np.int32)
    got = m.goal_paths(current, goals)
    td = ER.top_down(ER.states_to_bits(st), (X, Y, Z), 0, None)
    blocked = (td != 0).astype(np.int32)
    field, _ = PR.path_field(blocked, (2, 1))
    paths, offsets, lengths = PR.trace_many(field[None], np.concatenate([np.zeros((6, 1), np.int32), goals], axis=1))
    np.testing.assert_array_equal(got["paths"], paths)
    np.testing.assert_array_equal(got["offsets"], offsets)
    cost = np.array([PR.field_costs(field)[x, z] if x < X else np.inf for x, z in goals]) * float(np.float32(vs))
    np.testing.assert_array_equal(got["lengths_m"], cost)
    assert got["lengths_m"].dtype == np.float64 and np.isfinite(cost[0]) and np.isinf(cost[1]) and cost[2] == 0.0 and np.isinf(cost[3:]).all()
    assert [7] in paths[offsets[0]:offsets[1]][paths[offsets[0]:offsets[1], 0] == 6][:, 1:].tolist()          # through the gap
    # unknown cells free to cross: the unknown cell becomes reachable, the walled corner stays closed
    loose = m.goal_paths(current, goals, unknown_blocked=False)
    field2, _ = PR.path_field((td == 1).astype(np.int32), (2, 1))
    cost2 = np.array([PR.field_costs(field2)[x, z] if x < X else np.inf for x, z in goals]) * float(np.float32(vs))
    np.testing.assert_array_equal(loose["lengths_m"], cost2)
    assert np.isfinite(cost2[3]) and np.isinf(cost2[1]) and np.isinf(cost2[4])
    sliced = m.goal_paths(current, goals, y_lo=3, y_hi=5)                                      # nothing but unknown there: only the source
    assert sliced["lengths_m"][2] == 0.0 and np.isinf(np.delete(sliced["lengths_m"], 2)).all()


# ------------------------------------------------------------------ determinism
def test_the_same_call_twice_gives_the_same_bytes():
    blocked = PR.seeded_map((65, 63), 11, 0.25)
    src = [(32, 31), (0, 0), (64, 62), (10, 50)]
    a, ia = gpu_fields(blocked, src)
    b, ib = gpu_fields(blocked, src)
    assert a.tobytes() == b.tobytes() and ia[:, 0].tobytes() == ib[:, 0].tobytes()
    goals = np.array([[f, x, y] for f in range(4) for x in range(0, 65, 3) for y in range(0, 63, 5)], np.int32)
    paths, offsets, _ = PR.trace_many(a, goals)
    p1, i1 = gpu_trace(a, goals, offsets, int(offsets[-1]))
    p2, i2 = gpu_trace(a, goals, offsets, int(offsets[-1]))
    assert p1.tobytes() == p2.tobytes() == paths.tobytes() and i1.tolist() == i2.tolist()
