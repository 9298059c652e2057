"""CPU-side checks of the planner grid search (csrc/planning.hip, apnrf_amd/planning.py): the three symbols are declared, exported and
bound; every argument error is refused with MNF_ERR_INVALID before anything touches a device; and the numpy restatement the GPU tests
compare against (tests/planning_ref.py) is held to the reference's own answers (tests/golden/planner_paths.npz, written by
tests/golden/make_golden_planner.py from the reference's Dijkstra class) and its order function to integer brute force."""
import ctypes
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import apnrf_amd
from apnrf_amd import _lib as L

import planning_ref as PR

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("mnf_path_field_bytes", "mnf_path_field", "mnf_path_trace")
CASES = ("small", "cut", "blocked_start", "rooms")
INVALID = -1


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as G
    G.build()
    return apnrf_amd.load_library()


@pytest.fixture(scope="module")
def paths(golden):
    return golden("planner_paths")


def case_of(g, name):
    return {k[len(name) + 1:]: g[k] for k in g.files if k.startswith(name + "_")}


# ------------------------------------------------------------------ the boundary
def test_symbols_declared_exported_and_bound(lib):
    header = open(os.path.join(REPO, "include", "mi355nerf.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    raw = ctypes.CDLL(L.lib_path())
    for s in SYMBOLS:
        assert re.search(r"\b" + s + r"\s*\(", code), f"{s} is not declared in include/mi355nerf.h"
        assert hasattr(raw, s), f"{s} is not exported"
        assert s in L.SIGNATURES
    assert L.SIGNATURES["mnf_path_field_bytes"][0] is ctypes.c_int64
    assert len(L.SIGNATURES["mnf_path_field"][1]) == 11 and len(L.SIGNATURES["mnf_path_trace"][1]) == 10
    assert header.count("typedef struct {") == 5                             # plain arguments: no new struct
    for cite in ("dijkstra.py:72-182", ":194-215", ":247-260", "planning_funcs.py:288-326"):
        assert cite in header, cite
    from apnrf_amd import planning
    for name in ("path_field", "field_costs", "trace_paths", "Dijkstra"):
        assert hasattr(planning, name)
    from apnrf_amd.explore import ExplorationMap
    assert hasattr(ExplorationMap, "goal_paths")


def test_no_cpu_fallback():
    from apnrf_amd.planning import Dijkstra, path_field
    with pytest.raises(L.MnfError):
        Dijkstra([0, 0, 0, 1, 1, 1], np.zeros((4, 4), np.int32), 0.2, 0.05, device="cpu")
    with pytest.raises(L.MnfError):
        path_field(np.zeros((4, 4), np.int32), [[0, 0]])                     # a host array: nothing runs on the CPU


def test_byte_function(lib):
    f = lib.mnf_path_field_bytes
    assert f(1, 1, 1) == 4 and f(1, 1, 7) == 28 and f(24, 20, 3) == 24 * 20 * 3 * 4
    assert f(198, 198, 1) == 198 * 198 * 4 and f(198, 198, 300) == 198 * 198 * 4 * 300        # the cap: 200 * 200 bordered cells
    assert f(98, 98, 1) > 0 and f(120, 120, 1) > 0 and f(135, 140, 1) > 0                     # the reference's three scenes at 0.2 m
    assert f(1, 13331, 1) == 13331 * 4 and f(1, 13332, 1) == 0                                # (1 + 2)(ny + 2) <= 40000
    for bad in [(199, 199, 1), (1, 40000, 1), (40000, 1, 1), (198, 199, 1), (0, 4, 1), (4, 0, 1), (-1, 4, 1), (4, -4, 1), (0, 0, 1), (4, 4, -1),
                (1 << 30, 1 << 30, 1)]:
        assert f(*bad) == 0, bad
    assert f(4, 4, 0) == 0
    for nx, ny, n in [(1, 1, 1), (198, 198, 2), (199, 199, 1), (1, 40000, 1), (0, 3, 1), (24, 20, 5)]:
        assert f(nx, ny, n) == PR.bytes_of(nx, ny, n)


def _field(lib, **over):
    """mnf_path_field with plausible (never dereferenced) device pointers; `over` replaces arguments by name."""
    a = dict(blocked=0x1000, n_maps=1, nx=24, ny=20, lim_x=24, lim_y=20, sources=0x2000, n_sources=3, field=0x3000, info=0x4000, stream=None)
    a.update(over)
    rc = lib.mnf_path_field(*a.values())
    return rc, lib.mnf_last_error().decode()


def _trace(lib, **over):
    a = dict(field=0x1000, n_fields=2, nx=24, ny=20, goals=0x2000, offsets=0x3000, n_goals=5, paths=0x4000, info=0x5000, stream=None)
    a.update(over)
    rc = lib.mnf_path_trace(*a.values())
    return rc, lib.mnf_last_error().decode()


@pytest.mark.parametrize("name", ["blocked", "sources", "field", "info"])
def test_field_refuses_null_required_pointer(lib, name):
    rc, msg = _field(lib, **{name: None})
    assert rc == INVALID and name in msg, (rc, msg)


def test_field_refuses_bad_arguments(lib):
    for over, word in [(dict(nx=0), "positive"), (dict(ny=-3), "positive"), (dict(nx=199, ny=199, lim_x=199, lim_y=199), "LDS"),
                       (dict(nx=1, ny=40000, lim_x=1, lim_y=40000), "LDS"), (dict(lim_x=25), "limits"), (dict(lim_y=21), "limits"),
                       (dict(lim_x=-1), "limits"), (dict(lim_y=-1), "limits"), (dict(n_sources=-1), "n_sources"), (dict(n_maps=2), "n_maps"),
                       (dict(n_maps=0), "n_maps"), (dict(n_maps=-1), "n_maps"), (dict(n_maps=4), "n_maps"), (dict(info=0x4004), "aligned")]:
        rc, msg = _field(lib, **over)
        assert rc == INVALID and word in msg, (over, rc, msg)


def test_field_of_no_source_is_ok(lib):
    assert _field(lib, n_sources=0)[0] == 0
    assert _field(lib, n_sources=0, blocked=None, sources=None, field=None, info=None)[0] == 0
    assert _field(lib, n_sources=0, n_maps=0)[0] == 0                        # n_maps == n_sources
    assert _field(lib, n_sources=0, nx=199, ny=199)[0] == INVALID            # the geometry is still checked


@pytest.mark.parametrize("name", ["field", "goals", "offsets", "paths", "info"])
def test_trace_refuses_null_required_pointer(lib, name):
    rc, msg = _trace(lib, **{name: None})
    assert rc == INVALID and name in msg, (rc, msg)


def test_trace_refuses_bad_arguments(lib):
    for over, word in [(dict(nx=0), "positive"), (dict(ny=0), "positive"), (dict(nx=-5), "positive"), (dict(nx=199, ny=199), "199 x 199"),
                       (dict(n_fields=-1), "n_fields"), (dict(n_goals=-1), "n_goals"), (dict(info=0x5004), "aligned"), (dict(offsets=0x3004), "aligned")]:
        rc, msg = _trace(lib, **over)
        assert rc == INVALID and word in msg, (over, rc, msg)


# ------------------------------------------------------------------ the order of the labels
def test_order_against_integer_brute_force():
    """All pairs of labels with a, b <= 40.  The brute force: da + db sqrt(2) < 0 decided on Fractions by squaring, with no shortcut for
    signs that agree; and float64 a + b sqrt(2), formed freshly, must order every pair the same way."""
    def brute(da, db):
        # sign of da + db * sqrt(2): compare da with -db * sqrt(2) through their squares, signs handled by hand
        lhs, rhs = Fraction(da), Fraction(-db)                               # da < rhs * sqrt(2)?
        if lhs == 0 and rhs == 0:
            return 0
        if lhs >= 0 and rhs <= 0:
            return 1
        if lhs <= 0 and rhs >= 0:
            return -1
        if lhs > 0:                                                          # both positive: da^2 against 2 db^2
            return 1 if lhs * lhs > 2 * rhs * rhs else -1
        return 1 if lhs * lhs < 2 * rhs * rhs else -1                        # both negative
    n = 41
    a, b = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    cost = (a.astype(np.float64) + b.astype(np.float64) * math.sqrt(2.0)).reshape(-1)
    pairs = [(int(x), int(y)) for x, y in zip(a.reshape(-1), b.reshape(-1))]
    signs = {}
    for da in range(-n + 1, n):
        for db in range(-n + 1, n):
            signs[(da, db)] = brute(da, db)
            assert PR.sign_cost(da, db) == signs[(da, db)], (da, db)
    checked = 0
    for i, p in enumerate(pairs):
        d = cost[i] - cost                                                   # float64, against every q at once
        want = np.array([signs[(p[0] - q[0], p[1] - q[1])] for q in pairs])
        assert (np.sign(d) == want).all(), p
        checked += len(pairs)
        assert PR.less(p, pairs[(i * 7 + 3) % len(pairs)]) == (want[(i * 7 + 3) % len(pairs)] < 0)
    assert checked == (n * n) ** 2
    assert len(set(cost.tolist())) == n * n                                  # no two labels cost the same
    assert sorted(PR.Key(*p) for p in [(0, 3), (4, 0), (1, 2), (3, 1)])[0] == PR.Key(1, 2)      # 3.83 < 4 < 4.24 < 4.41


# ------------------------------------------------------------------ the restatement against the reference's answers
@pytest.fixture(scope="module")
def restated(paths):
    out = {}
    for name in CASES:
        c = case_of(paths, name)
        lim = PR.limits_of(c["aabb"].tolist(), c["map"].shape, float(c["res"]))
        field, reached = PR.path_field(c["map"], c["start_cell"], lim)
        out[name] = (c, lim, field, reached)
    return out


def test_fixture_holds_what_the_tests_rely_on(restated):
    c, lim, field, reached = restated["small"]
    nx, ny = c["map"].shape
    assert (nx, ny) == (24, 20) and lim == (24, 20) and c["goals"].shape == (482, 2)
    free = c["map"] == 0
    none = c["none"][:480].reshape(nx, ny)
    assert (none & free).sum() >= 0.05 * free.sum() and (~none).sum() >= 0.25 * free.sum()
    assert 0.2 < (c["map"] != 0).mean() < 0.45
    assert c["none"][480:].all() and not (0 <= c["goal_cells"][480, 0] < nx) and c["goal_cells"][481, 0] < 0
    start = tuple(c["start_cell"])
    assert c["len"][start[0] * ny + start[1]] == 1 and c["ab"][start[0] * ny + start[1]].tolist() == [0, 0]
    assert restated["cut"][1] == (22, 20) and restated["cut"][0]["none"].reshape(nx, ny)[22:].all()
    b = restated["blocked_start"][0]
    assert b["map"][tuple(b["start_cell"])] != 0 and not b["none"][-1]
    r = restated["rooms"][0]
    assert r["map"].shape == (98, 98) and r["goals"].shape == (40, 2) and r["none"].sum() >= 6 and (~r["none"]).sum() >= 25


@pytest.mark.parametrize("name", CASES)
def test_restatement_equals_the_reference(restated, name):
    c, lim, field, reached = restated[name]
    nx, ny = c["map"].shape
    a, b, ok = PR.split(field)
    assert reached == ok.sum()
    n_reached = 0
    for g, (gx, gy) in enumerate(c["goal_cells"]):
        inside = 0 <= gx < nx and 0 <= gy < ny
        mine_none = not inside or not ok[gx, gy]
        assert mine_none == bool(c["none"][g]), (name, g, gx, gy)            # the None sets are equal
        cells = PR.trace(field, (gx, gy))
        if mine_none:
            assert cells.shape == (0, 2)
            continue
        n_reached += 1
        assert [a[gx, gy], b[gx, gy]] == c["ab"][g].tolist(), (name, g)      # the labels are the reference's make-up
        assert cells.shape[0] == c["len"][g] == a[gx, gy] + b[gx, gy] + 1
        assert PR.make_up(cells) == tuple(c["ab"][g].tolist())               # steps to 8-neighbours only
        assert tuple(cells[0]) == (gx, gy) and tuple(cells[-1]) == tuple(c["start_cell"])
        inner = cells[:-1]                                                   # every cell but the start was moved TO: legal
        assert (c["map"][inner[:, 0], inner[:, 1]] == 0).all() and (inner[:, 0] < lim[0]).all() and (inner[:, 1] < lim[1]).all()
    assert n_reached > 10


def test_restatement_trace_rule_and_costs():
    """A free 5 x 4 map from (1, 1): the closed form, the first matching move of the motion order, and the costs."""
    field, reached = PR.path_field(np.zeros((5, 4), np.int32), (1, 1))
    assert reached == 20
    a, b, ok = PR.split(field)
    for x in range(5):
        for y in range(4):
            dx, dy = abs(x - 1), abs(y - 1)
            assert (a[x, y], b[x, y]) == (abs(dx - dy), min(dx, dy))
    # (4, 3): label (1, 2).  Motion order: (1, 0) comes first, and (3, 3) carries (0, 2): the straight step is taken first
    assert PR.trace(field, (4, 3)).tolist() == [[4, 3], [3, 3], [2, 2], [1, 1]]
    assert PR.trace(field, (1, 1)).tolist() == [[1, 1]] and PR.trace(field, (5, 0)).shape == (0, 2) and PR.trace(field, (0, -1)).shape == (0, 2)
    costs = PR.field_costs(field)
    assert costs[4, 3] == 1.0 + 2.0 * math.sqrt(2.0) and costs[1, 1] == 0.0
    walled = np.zeros((3, 3), np.int32)
    walled[1, :] = 1
    f, n = PR.path_field(walled, (0, 0))
    assert n == 3 and np.isinf(PR.field_costs(f)[2]).all() and (f[1] == PR.UNREACHED).all()
    f, n = PR.path_field(walled, (1, 1))                                     # a blocked source has cost 0 and is left freely
    assert n == 7 and f[1, 1] == 0 and f[1, 0] == PR.UNREACHED and f[0, 0] == 1 and f[2, 1] == 1 << 16
    f, n = PR.path_field(walled, (3, 0))
    assert n == 0 and (f == PR.UNREACHED).all()
    paths, offsets, lengths = PR.trace_many(field[None], [[0, 4, 3], [0, 9, 9], [1, 0, 0], [0, 1, 1]])
    assert lengths.tolist() == [4, 0, 0, 1] and offsets.tolist() == [0, 4, 4, 4, 5] and paths.shape == (5, 2)


def test_map_builders():
    s = PR.serpentine(9)
    f, n = PR.path_field(s, (0, 0))
    a, b, ok = PR.split(f)
    assert n == (s == 0).sum() and ok[8, 0] and a[8, 0] + b[8, 0] >= 4 * 6            # every corridor is crossed from column <= 1 to column >= 7
    r = PR.rooms_map(98, 14)
    f, n = PR.path_field(r, (49, 49))
    assert (f[:14, :14] == PR.UNREACHED).all() and n == (r == 0).sum() - 14 * 14
