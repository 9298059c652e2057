"""CPU-side checks of the planner cost map and goal draw (csrc/scanmap.hip, apnrf_amd/planning.py): the four symbols are declared,
exported and bound; every argument error is refused with MNF_ERR_INVALID before anything touches a device; and the numpy restatement the
GPU tests compare against (tests/scanmap_ref.py) is held to the reference's own answers (tests/golden/scan_maps.npz, written by
tests/golden/make_golden_scanmap.py from the reference's update_cost_map), its closed-form column to the running error term, and the
closed-form yaw to scipy's values."""
import ctypes
import os
import re

import numpy as np
import pytest

import apnrf_amd
from apnrf_amd import _lib as L

import scanmap_ref as SR

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("mnf_scan_map_bytes", "mnf_scan_map_update", "mnf_planner_goal_map", "mnf_planner_goal_pick")
CASES = ("small", "wide")
INVALID = -1


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as G
    G.build()
    return apnrf_amd.load_library()


@pytest.fixture(scope="module")
def maps(golden):
    return golden("scan_maps")


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
    assert L.SIGNATURES["mnf_scan_map_bytes"][0] is ctypes.c_int64
    assert [len(L.SIGNATURES[s][1]) for s in SYMBOLS] == [2, 15, 11, 7]
    assert header.count("typedef struct {") == 5                             # plain arguments: no new struct
    for cite in ("planning_funcs.py:192-219", "depth_to_grid.py:31-73", ":142-182", "pipeline.py:272-292", ":1115-1138", ":1171-1189",
                 "planning_funcs.py:262-276", "planning_funcs.py:296-326", "one\n * deliberate difference"):
        assert cite in header, cite
    from apnrf_amd import planning
    for name in ("ScanCostMap", "goal_cells", "draw_goals", "align_angles", "yaw_of"):
        assert hasattr(planning, name)
    for name in ("update", "update_dataset", "cost_map", "visiting_map", "info", "clear"):
        assert hasattr(planning.ScanCostMap, name)


def test_no_cpu_fallback():
    import torch
    from apnrf_amd.planning import ScanCostMap, draw_goals, goal_cells
    with pytest.raises(L.MnfError):
        ScanCostMap([0, 0, 0, 2, 1, 2], 0.2, device="cpu")
    with pytest.raises(L.MnfError):
        goal_cells(np.zeros((4, 5), np.int32), np.zeros((4, 5), np.int32))   # host arrays: nothing runs on the CPU
    with pytest.raises(L.MnfError):
        draw_goals(torch.zeros(20, 2, dtype=torch.int32), torch.zeros(1, dtype=torch.int64), [0.5])


def test_byte_function(lib):
    f = lib.mnf_scan_map_bytes
    assert f(1, 1) == 12 and f(5, 4) == 240 and f(24, 20) == 3 * 24 * 20 * 4
    assert f(198, 198) == 3 * 198 * 198 * 4 and f(98, 98) > 0 and f(135, 140) > 0        # the cap: 200 * 200 bordered cells
    assert f(1, 13331) == 3 * 13331 * 4 and f(1, 13332) == 0
    for bad in [(199, 199), (198, 199), (1, 40000), (40000, 1), (0, 4), (4, 0), (-1, 4), (4, -4), (1 << 30, 1 << 30)]:
        assert f(*bad) == 0, bad
    for nx, nz in [(1, 1), (198, 198), (199, 199), (0, 3), (24, 20), (1, 13332)]:
        assert f(nx, nz) == SR.state_bytes(nx, nz)


AABB = (ctypes.c_double * 6)(-2.0, -0.5, -1.6, 2.8, 2.5, 2.4)


def _update(lib, **over):
    """mnf_scan_map_update with plausible (never dereferenced) device pointers; `over` replaces arguments by name."""
    a = dict(state=0x1000, nx=24, nz=20, depth=0x2000, n_views=3, height=4, width=64, align=0x3000, yaw=0x4000, loc=0x5000, centre=0x6000,
             aabb_host=AABB, res=0.2, info=0x7000, stream=None)
    a.update(over)
    rc = lib.mnf_scan_map_update(*a.values())
    return rc, lib.mnf_last_error().decode()


def _goal_map(lib, **over):
    a = dict(blocked=0x1000, visits=0x2000, field=0x3000, nx=24, nz=20, decay=0x4000, n_decay=16, vm=0x5000, cells=0x6000, count=0x7000, stream=None)
    a.update(over)
    rc = lib.mnf_planner_goal_map(*a.values())
    return rc, lib.mnf_last_error().decode()


def _goal_pick(lib, **over):
    a = dict(cells=0x1000, count=0x2000, max_cells=480, u=0x3000, n_draws=5, goals=0x4000, stream=None)
    a.update(over)
    rc = lib.mnf_planner_goal_pick(*a.values())
    return rc, lib.mnf_last_error().decode()


@pytest.mark.parametrize("name", ["state", "depth", "align", "yaw", "loc", "centre", "aabb_host", "info"])
def test_update_refuses_null_required_pointer(lib, name):
    rc, msg = _update(lib, **{name: None})
    assert rc == INVALID and name in msg, (rc, msg)


def test_update_refuses_bad_arguments(lib):
    nan6 = (ctypes.c_double * 6)(-2.0, -0.5, float("nan"), 2.8, 2.5, 2.4)
    inf6 = (ctypes.c_double * 6)(float("inf"), -0.5, -1.6, 2.8, 2.5, 2.4)
    for over, word in [(dict(nx=0), "positive"), (dict(nz=-3), "positive"), (dict(nx=199, nz=199), "LDS"), (dict(nx=1, nz=40000), "LDS"),
                       (dict(n_views=-1), "n_views"), (dict(n_views=(1 << 20) + 1), "n_views"), (dict(height=0), "height"), (dict(height=-2), "height"),
                       (dict(width=0), "width"), (dict(width=-1), "width"), (dict(width=(1 << 24) + 1), "width"), (dict(res=0.0), "res"),
                       (dict(res=-0.2), "res"), (dict(res=float("nan")), "res"), (dict(res=float("inf")), "res"), (dict(aabb_host=nan6), "aabb[2]"),
                       (dict(aabb_host=inf6), "aabb[0]"), (dict(info=0x7004), "aligned"), (dict(align=0x3004), "aligned"), (dict(yaw=0x4004), "aligned"),
                       (dict(loc=0x5004), "aligned"), (dict(centre=0x6002), "aligned"), (dict(depth=0x2001), "aligned"), (dict(state=0x1002), "aligned")]:
        rc, msg = _update(lib, **over)
        assert rc == INVALID and word in msg, (over, rc, msg)


def test_update_of_no_view_is_ok(lib):
    assert _update(lib, n_views=0)[0] == 0
    assert _update(lib, n_views=0, depth=None, align=None, yaw=None, loc=None, centre=None)[0] == 0
    assert _update(lib, n_views=0, nx=199, nz=199)[0] == INVALID             # the geometry is still checked
    assert _update(lib, n_views=0, state=None)[0] == INVALID


@pytest.mark.parametrize("name", ["blocked", "visits", "decay", "vm", "cells", "count"])
def test_goal_map_refuses_null_required_pointer(lib, name):
    rc, msg = _goal_map(lib, **{name: None})
    assert rc == INVALID and name in msg, (rc, msg)


def test_goal_map_refuses_bad_arguments(lib):
    for over, word in [(dict(nx=0), "positive"), (dict(nz=0), "positive"), (dict(nx=-5), "positive"), (dict(nx=199, nz=199), "cap"),
                       (dict(n_decay=0), "n_decay"), (dict(n_decay=-4), "n_decay"), (dict(decay=0x4004), "aligned"), (dict(vm=0x5004), "aligned"),
                       (dict(count=0x7004), "aligned")]:
        rc, msg = _goal_map(lib, **over)
        assert rc == INVALID and word in msg, (over, rc, msg)


@pytest.mark.parametrize("name", ["cells", "count", "u", "goals"])
def test_goal_pick_refuses_null_required_pointer(lib, name):
    rc, msg = _goal_pick(lib, **{name: None})
    assert rc == INVALID and name in msg, (rc, msg)


def test_goal_pick_refuses_bad_arguments_and_takes_no_draw(lib):
    for over, word in [(dict(max_cells=-1), "max_cells"), (dict(max_cells=40001), "max_cells"), (dict(n_draws=-1), "n_draws"),
                       (dict(n_draws=1 << 31), "n_draws"), (dict(count=0x2004), "aligned"), (dict(u=0x3004), "aligned")]:
        rc, msg = _goal_pick(lib, **over)
        assert rc == INVALID and word in msg, (over, rc, msg)
    assert _goal_pick(lib, n_draws=0)[0] == 0
    assert _goal_pick(lib, n_draws=0, u=None, goals=None)[0] == 0
    assert _goal_pick(lib, n_draws=0, count=None)[0] == INVALID


# ------------------------------------------------------------------ the restatement against the reference's answers
@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("use_loop", [False, True])
def test_restatement_equals_the_reference(maps, name, use_loop):
    c = case_of(maps, name)
    shape = tuple(int(v) for v in c["shape"])
    H = c["depth"].shape[1]
    codes, visits = np.zeros(shape, np.int32), np.zeros(shape, np.int32)
    aabb = c["aabb"].astype(np.float64)
    seen = []

    def after(v, codes, visits):
        assert np.array_equal(SR.cost_map(codes), c["cost"][v]), v
        assert np.array_equal(visits.astype(np.float64), c["visiting"][v]), v
        seen.append(v)

    info = SR.scan_update(codes, visits, c["depth"][:, H // 2], c["align"], c["yaw"], c["poses"][:, [0, 2], 3], c["centre"], aabb, float(c["res"]),
                          use_loop=use_loop, after_each=after)
    assert seen == list(range(len(c["yaw"])))
    assert info.tolist() == [0, 0, 0, c["depth"].shape[0] * c["depth"].shape[2]]      # the fixture never leaves on the low side


@pytest.mark.parametrize("name", CASES)
def test_host_inputs_equal_the_reference(maps, name):
    """What ScanCostMap forms on the host (yaw in closed form, centre cells, align angles) against the generator's scipy and numpy values."""
    from apnrf_amd import planning
    c = case_of(maps, name)
    assert np.abs(planning.yaw_of(c["poses"]) - c["yaw"]).max() <= 1e-12
    assert np.abs(SR.yaw_of(c["poses"]) - c["yaw"]).max() <= 1e-12
    assert np.array_equal(SR.centre_of(c["poses"], c["aabb"], float(c["res"])), c["centre"])
    W = c["depth"].shape[2]
    assert np.array_equal(planning.align_angles(W), c["align"])
    assert np.array_equal(SR.align_angles(W), c["align"])
    for bad in (0, -2, 7):
        with pytest.raises(ValueError):
            planning.align_angles(bad)


def test_align_angles_are_the_pipelines_at_640():
    from apnrf_amd import planning
    r = np.arctan(np.linspace(0.5, 319.5, 320) / 320).tolist()
    r.reverse()
    l = np.arctan(-np.linspace(0.5, 319.5, 320) / 320).tolist()
    assert np.array_equal(planning.align_angles(640), np.array(r + l))


ENDS = [(7, 3), (3, 7), (-7, 3), (-3, 7), (-7, -3), (-3, -7), (7, -3), (3, -7),       # the 8 octants
        (9, 0), (-9, 0), (0, 9), (0, -9), (5, 5), (-5, 5), (5, -5), (-5, -5),        # the axes and the diagonals
        (0, 0), (1, 0), (0, 1), (1, 1), (2, 1), (1, 2), (40, 39), (39, 40), (101, 7), (7, 101), (-101, 50), (64, -33)]


@pytest.mark.parametrize("start", [(0, 0), (4, 9), (-3, 2)])
def test_closed_form_column_equals_the_loop(start):
    for ex, ey in ENDS:
        end = (start[0] + ex, start[1] + ey)
        loop, closed = SR.walk_loop(start, end), SR.walk_closed(start, end)
        assert np.array_equal(loop, closed), (start, end)
        assert len(loop) == max(abs(ex), abs(ey)) + 1
        assert {tuple(loop[0]), tuple(loop[-1])} == {start, end}
        shape = (12, 9)
        inside = loop[(loop[:, 0] >= 0) & (loop[:, 0] < shape[0]) & (loop[:, 1] >= 0) & (loop[:, 1] < shape[1])]
        assert np.array_equal(SR.walk_closed(start, end, shape), inside), (start, end)


def test_closed_form_column_equals_the_loop_at_random():
    rng = np.random.default_rng(2)
    for _ in range(300):
        s, e = tuple(int(v) for v in rng.integers(-30, 60, 2)), tuple(int(v) for v in rng.integers(-30, 60, 2))
        assert np.array_equal(SR.walk_loop(s, e), SR.walk_closed(s, e)), (s, e)


def test_a_far_beam_costs_the_grid_not_the_depth():
    cells = SR.walk_closed((3, 4), (3 + (1 << 29), 4 + (1 << 28)), (20, 16))
    assert 0 < len(cells) <= 20
    assert np.array_equal(cells, SR.walk_loop((3, 4), (3 + 64, 4 + 32))[:len(cells)])   # the same slope: the first columns agree


def test_skip_policy_of_the_restatement():
    shape, aabb, res = (6, 5), np.array([0.0, 0.0, 0.0, 1.2, 1.0, 1.0]), 0.2
    align = np.zeros(6)
    depth = np.array([0.4, np.nan, np.inf, -np.inf, 1e4, 3e9], np.float32)
    info = np.zeros(4, np.int64)
    plane = SR.scan_view(shape, depth, align, np.pi, (0.45, 0.45), (2, 2), aabb, res, info)   # yaw pi: the beams run towards +z
    assert info.tolist() == [0, 3, 1, 2]
    assert (plane[2, 2:] == 0).sum() >= 2 and plane[2, 4] in (0, 1)
    info[:] = 0
    SR.scan_view(shape, depth[:1], align[:1], 0.0, (0.45, 0.45), (2, 2), aabb, res, info)     # yaw 0: towards -z, still inside
    assert info.tolist() == [0, 0, 0, 1]
    info[:] = 0
    SR.scan_view(shape, np.array([0.8], np.float32), align[:1], 0.0, (0.45, 0.45), (2, 2), aabb, res, info)
    assert info.tolist() == [1, 0, 0, 1]


def test_vm_and_goal_list_of_the_restatement():
    rng = np.random.default_rng(4)
    blocked = (rng.random((7, 5)) < 0.4).astype(np.int32)
    visits = rng.integers(2, 9, (7, 5)).astype(np.int32)
    vm = SR.vm_of(blocked, visits)
    ref = visits.astype(np.float64)                                          # planning_funcs.py:268-276, spelt out
    ref[(blocked > 1e-4) == 1] = -1
    ref[(blocked > 1e-4) == 0] = np.exp(-(ref[(blocked > 1e-4) == 0] - np.min(ref[(blocked > 1e-4) == 0])) / 5)
    assert np.array_equal(vm, ref) and vm.max() == 1.0
    assert np.array_equal(SR.goal_list(vm), np.argwhere(vm >= 0))
    assert SR.goal_list(SR.vm_of(np.ones((3, 4), np.int32), np.zeros((3, 4), np.int32))).shape == (0, 2)
    cells = SR.goal_list(vm)
    n = len(cells)
    assert np.array_equal(SR.pick(cells, n, [0.0, np.nextafter(1.0, 0.0), 1.0 / n, np.nextafter(1.0 / n, 0.0)]), cells[[0, n - 1, 1, 0]])
    from apnrf_amd import planning
    table = planning._decay_table()
    assert table[0] == 1.0 and table[-1] == 0.0 and table[3727] == 0.0 and np.array_equal(table[:40], np.exp(-np.arange(40.0) / 5))
