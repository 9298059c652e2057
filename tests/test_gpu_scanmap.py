"""GPU tests of the planner cost map and goal draw (csrc/scanmap.hip, apnrf_amd/planning.py) against the reference's own maps
(tests/golden/scan_maps.npz) and against the numpy restatement tests/scanmap_ref.py, which tests/test_scanmap_cpu.py holds to those maps.
Every comparison is `array_equal`: cost codes, visit counts, info, vm, cells and count.  Outputs of the C ABI are allocated with canaries
on both sides.  Depths are moved off the half-integer end coordinates first (scanmap_ref.settle_depths), so a last-bit difference
between the device's sin / cos and libm's cannot move an end cell."""
import ctypes

import numpy as np
import pytest
import torch

import scanmap_ref as SR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CANARY = 64
MARK32, MARK64 = -0x5A5A5A5B, -0x5A5A5A5A5A5A5A5B
MARKF = -7.25
CASES = ("small", "wide")
AABB = np.array([0.0, -0.5, 0.0, 1.0, 2.5, 0.8])          # the 5 x 4 grid at 0.2 m
AABB_Q = np.array([0.2, -0.5, -0.4, 1.2, 2.5, 0.4])       # aabb[0] != aabb[2]: x cells from x - aabb[2], z cells from z - aabb[0]
RES = 0.2


def _dev(a):
    return torch.from_numpy(np.array(a, copy=True, order="C")).to(DEV)


def case_of(g, name):
    return {k[len(name) + 1:]: g[k] for k in g.files if k.startswith(name + "_")}


@pytest.fixture(scope="module")
def fixture(golden):
    g = golden("scan_maps")
    return {name: case_of(g, name) for name in CASES}


def _guarded(n, dtype, mark):
    whole = torch.full((n + 2 * CANARY,), mark, dtype=dtype, device=DEV)
    return whole, whole[CANARY:CANARY + n]


def _assert_guards(whole, n, mark, what):
    host = whole.cpu().numpy()
    assert (host[:CANARY] == mark).all() and (host[CANARY + n:] == mark).all(), f"{what}: written outside its bounds"


class AbiMap:
    """A cost map held through the C ABI alone: the state between canaries, info accumulated."""

    def __init__(self, shape):
        from apnrf_amd import _lib as L
        self.L, self.lib = L, L.load_library()
        self.nx, self.nz = shape
        self.n = 3 * self.nx * self.nz
        assert self.lib.mnf_scan_map_bytes(self.nx, self.nz) == 4 * self.n
        self.whole, self.state = _guarded(self.n, torch.int32, MARK32)
        self.state.zero_()
        self.iw, self.info = _guarded(4, torch.int64, MARK64)
        self.info.zero_()

    def update(self, depth, align, yaws, locs, centres, aabb, res):
        L = self.L
        depth = np.asarray(depth, np.float32)
        V, H, W = depth.shape
        d_depth, d_align, d_yaw = _dev(depth), _dev(np.asarray(align, np.float64)), _dev(np.asarray(yaws, np.float64))
        d_loc, d_centre = _dev(np.asarray(locs, np.float64).reshape(V, 2)), _dev(np.asarray(centres, np.int32).reshape(V, 2))
        box = (ctypes.c_double * 6)(*[float(v) for v in aabb])
        L.launch(self.lib.mnf_scan_map_update, L.ptr(self.state), self.nx, self.nz, L.ptr(d_depth), V, H, W, L.ptr(d_align), L.ptr(d_yaw), L.ptr(d_loc),
                 L.ptr(d_centre), box, float(res), L.ptr(self.info), device=torch.device(DEV))
        torch.cuda.synchronize()
        _assert_guards(self.whole, self.n, MARK32, "state")
        _assert_guards(self.iw, 4, MARK64, "info")

    def read(self):
        s = self.state.cpu().numpy().reshape(3, self.nx, self.nz)
        return s[0].copy(), s[1].copy(), self.info.cpu().numpy().copy()


def images_of(rows, H=3, seed=0):
    """[V,H,W] float32 with `rows` [V,W] at row H // 2 and other depths everywhere else: only the middle row may be read."""
    rows = np.asarray(rows, np.float32)
    d = np.random.default_rng(seed).uniform(0.1, 9.0, (rows.shape[0], H, rows.shape[1])).astype(np.float32)
    d[:, H // 2] = rows
    return d


def check(shape, rows, align, yaws, locs, centres, aabb=AABB, res=RES, settle=True, H=3, amap=None):
    """One batch through the C ABI against the restatement (which starts from the same earlier state) -> (codes, visits, info)."""
    rows = np.asarray(rows, np.float32).reshape(len(yaws), -1)
    locs, centres = np.asarray(locs, np.float64).reshape(-1, 2), np.asarray(centres, np.int64).reshape(-1, 2)
    if settle:
        rows = SR.settle_depths(rows, align, yaws, locs, aabb, res)
    amap = AbiMap(shape) if amap is None else amap
    codes, visits, info = amap.read()
    amap.update(images_of(rows, H), align, yaws, locs, centres, aabb, res)
    SR.scan_update(codes, visits, rows, align, yaws, locs, centres, aabb, res, info=info)
    got = amap.read()
    np.testing.assert_array_equal(got[0], codes)
    np.testing.assert_array_equal(got[1], visits)
    np.testing.assert_array_equal(got[2], info)
    return got


OCTANTS = np.arange(8) * (np.pi / 4) + 0.2


# ------------------------------------------------------------------ the reference's own maps
@pytest.mark.parametrize("name", CASES)
def test_goldens_through_the_c_abi(fixture, name):
    c = fixture[name]
    shape = tuple(int(v) for v in c["shape"])
    aabb, res, locs = c["aabb"].astype(np.float64), float(c["res"]), c["poses"][:, [0, 2], 3]
    one, batch = AbiMap(shape), AbiMap(shape)
    V = len(c["yaw"])
    for v in range(V):                                                               # view after view: the reference's maps after each
        one.update(c["depth"][v:v + 1], c["align"], c["yaw"][v:v + 1], locs[v:v + 1], c["centre"][v:v + 1], aabb, res)
        codes, visits, _ = one.read()
        np.testing.assert_array_equal(SR.cost_map(codes), c["cost"][v])
        np.testing.assert_array_equal(visits.astype(np.float64), c["visiting"][v])
    batch.update(c["depth"], c["align"], c["yaw"], locs, c["centre"], aabb, res)
    for a, b in zip(one.read(), batch.read()):
        np.testing.assert_array_equal(a, b)
    assert one.read()[2].tolist() == [0, 0, 0, V * c["depth"].shape[2]]


@pytest.mark.parametrize("name", CASES)
def test_goldens_through_scan_cost_map(fixture, name):
    from apnrf_amd.planning import ScanCostMap
    c = fixture[name]
    shape = tuple(int(v) for v in c["shape"])
    m = ScanCostMap(c["aabb"], float(c["res"]), device=DEV)
    assert (m.nx, m.nz) == shape                                                     # the reference's main_grid_resolution
    assert np.array_equal(m.cost_map().cpu().numpy(), np.full(shape, 0.5)) and not m.visiting_map().any()
    V = len(c["yaw"])
    m.update(c["depth"][:2], c["poses"][:2])                                         # host arrays
    assert m.cost_map().dtype == torch.float64 and m.visiting_map().dtype == torch.float64
    np.testing.assert_array_equal(m.cost_map().cpu().numpy(), c["cost"][1])
    np.testing.assert_array_equal(m.visiting_map().cpu().numpy(), c["visiting"][1])
    m.update(_dev(c["depth"][2:]), _dev(c["poses"][2:]), align_angles=c["align"])    # device tensors, explicit angles
    np.testing.assert_array_equal(m.cost_map().cpu().numpy(), c["cost"][V - 1])
    np.testing.assert_array_equal(m.visiting_map().cpu().numpy(), c["visiting"][V - 1])
    assert m.info() == {"negative_cell": 0, "bad_depth": 0, "far": 0, "drawn": V * c["depth"].shape[2]}
    yaw, loc, centre = m.view_inputs(c["poses"])
    assert np.array_equal(centre, c["centre"]) and np.array_equal(loc, c["poses"][:, [0, 2], 3])
    m.clear()
    assert np.array_equal(m.cost_map().cpu().numpy(), np.full(shape, 0.5)) and not m.visiting_map().any() and m.info()["drawn"] == 0


class _Stored:
    """The attributes of a Dataset that update_dataset reads."""

    def __init__(self, depth, poses):
        self.depths, self.camtoworlds = _dev(depth.reshape(depth.shape[0], -1)), _dev(poses.astype(np.float32))
        self.height, self.width = depth.shape[1:]

    def __len__(self):
        return int(self.depths.shape[0])


def test_update_dataset_reads_the_stored_views(fixture):
    from apnrf_amd.planning import ScanCostMap
    c = fixture["small"]
    poses32 = c["poses"].astype(np.float32).astype(np.float64)                       # a Dataset stores float32 poses
    ids = [3, 0, 4]
    m, want = ScanCostMap(c["aabb"], float(c["res"]), device=DEV), ScanCostMap(c["aabb"], float(c["res"]), device=DEV)
    m.update_dataset(_Stored(c["depth"], c["poses"]), ids)
    want.update(c["depth"][ids], poses32[ids])
    assert want.info()["drawn"] == 3 * c["depth"].shape[2]
    assert torch.equal(m.state, want.state) and m.info() == want.info()


# ------------------------------------------------------------------ against the restatement
def test_one_beam():
    codes, _, info = check((5, 4), [[0.35]], [0.3], [2.0], [(0.45, 0.35)], [(2, 1)])
    assert info.tolist() == [0, 0, 0, 1] and (codes == 2).any() and (codes == 1).any()


@pytest.mark.parametrize("aabb", [AABB, AABB_Q])
def test_one_beam_per_octant(aabb):
    codes, visits, info = check((5, 4), [[0.5] * 8], OCTANTS, [0.1], [(0.45, 0.45)], [(2, 2)], aabb=aabb)
    assert info[3] == 8 and codes[2, 2] == 1 and visits.max() == 1


def test_zero_length_beam():
    codes, visits, info = check((5, 4), [[0.0]], [0.7], [0.4], [(0.45, 0.45)], [(2, 2)], settle=False)
    assert info.tolist() == [0, 0, 0, 1]
    assert codes[2, 2] == 2 and codes[3, 3] == 2 and (codes == 2).sum() == 4 and not visits.any()      # the walk's one cell is stamped over


def test_centre_on_each_border_and_outside():
    centres = [(0, 2), (4, 2), (2, 0), (2, 3), (0, 0), (4, 3), (-2, 1), (7, 2), (2, -3), (1, 6)]
    locs = [(0.2 * x + 0.05, 0.2 * z + 0.05) for x, z in centres]
    V = len(centres)
    _, _, info = check((5, 4), [[0.5] * 8] * V, OCTANTS, np.linspace(-3, 3, V), locs, centres)
    assert info[3] == 8 * V and info[0] >= 16                                        # the two centres with a negative index count every beam


def test_beams_leaving_on_the_high_and_low_side():
    yaws, locs = [0.0, 0.5], [(0.45, 0.45), (0.3, 0.5)]
    rows = SR.settle_depths(np.float32([[3.0] * 8, [1.1] * 8]), OCTANTS, yaws, locs, AABB, RES)
    _, _, info = check((5, 4), rows, OCTANTS, yaws, locs, [(2, 2), (1, 2)], settle=False)
    low = high = 0
    for v in range(2):
        fx, fy = SR.end_coordinates(rows[v], OCTANTS, yaws[v], locs[v], AABB, RES)
        low += int(((np.rint(fx) < 0) | (np.rint(fy) < 0)).sum())
        high += int(((np.rint(fx) >= 5) | (np.rint(fy) >= 4)).sum())
    assert info[0] == low and 0 < low < 16 and high > 4 and info[3] == 16            # some leave on the low side, some on the high side


def test_far_and_bad_depths():
    rows = [[0.5, 1e4, np.nan, np.inf, 0.3, -np.inf, 3e9, 1e30]]
    _, _, info = check((5, 4), rows, OCTANTS[[1, 1, 2, 3, 4, 5, 6, 7]], [0.3], [(0.45, 0.45)], [(2, 2)])
    assert info[1] == 3 and info[2] == 2 and info[3] == 3
    # a NaN yaw, a location that is not finite, a centre beyond 2^30: nothing of those views is drawn
    _, _, info = check((5, 4), [[0.5] * 8] * 4, OCTANTS, [0.0, np.nan, 0.2, 0.3], [(0.45, 0.45), (0.45, 0.45), (np.inf, 0.2), (0.45, 0.45)],
                       [(2, 2), (2, 2), (2, 2), ((1 << 30) + 1, 2)])
    assert info.tolist()[1:] == [0, 24, 8]


def test_order_within_a_view():
    # yaw pi: both beams run from the cell (2, 0) towards +z on a 5 x 8 grid
    aabb = np.array([0.0, -0.5, 0.0, 1.0, 2.5, 1.6])
    codes, _, _ = check((5, 8), [[0.4, 1.2]], [0.0, 0.0], [np.pi], [(0.45, 0.05)], [(2, 0)], aabb=aabb)
    assert codes[2, 2] == 1 and codes[2, 3] == 1 and codes[3, 2] == 2                # occupied by beam 0, freed by beam 1
    assert codes[2, 6] == 2
    codes, _, _ = check((5, 8), [[1.2, 0.4]], [0.0, 0.0], [np.pi], [(0.45, 0.05)], [(2, 0)], aabb=aabb)
    assert codes[2, 2] == 2 and codes[2, 3] == 2 and codes[2, 1] == 1                # freed by beam 0, occupied by beam 1
    assert codes[2, 6] == 2 and codes[2, 4] == 1


def _random_views(rng, shape, V, W, res, depth_range):
    nx, nz = shape
    aabb = np.array([-0.3, -0.5, 0.1, -0.3 + nx * res, 2.5, 0.1 + nz * res])
    # x cells come from world x - aabb[2], z cells from world z - aabb[0]; the centres are put where the beams start
    locs = np.stack([aabb[2] + rng.uniform(0.3, 0.7, V) * nx * res, aabb[0] + rng.uniform(0.3, 0.7, V) * nz * res], axis=1)
    centres = np.stack([(locs[:, 0] - aabb[2]) // res, (locs[:, 1] - aabb[0]) // res], axis=1).astype(np.int64)
    rows = rng.uniform(*depth_range, (V, W)).astype(np.float32)
    return aabb, locs, centres, rows, rng.uniform(-3, 3, V)


def test_batch_equals_one_call_per_view():
    rng = np.random.default_rng(21)
    shape, V, W = (13, 11), 3, 32
    aabb, locs, centres, rows, _ = _random_views(rng, shape, V, W, RES, (0.2, 1.4))
    locs = locs[:1] + np.array([[0.0, 0.0], [0.1, -0.1], [-0.15, 0.05]])             # three nearby cameras looking much the same way
    centres = np.stack([(locs[:, 0] - aabb[2]) // RES, (locs[:, 1] - aabb[0]) // RES], axis=1).astype(np.int64)
    yaws = np.array([0.3, 0.45, 0.6])
    align = SR.align_angles(W)
    rows = SR.settle_depths(rows, align, yaws, locs, aabb, RES)
    batch = AbiMap(shape)
    got = check(shape, rows, align, yaws, locs, centres, aabb=aabb, settle=False, amap=batch)
    assert got[1].max() >= 2                                                         # the views overlap
    single = AbiMap(shape)
    for v in range(V):
        check(shape, rows[v:v + 1], align, yaws[v:v + 1], locs[v:v + 1], centres[v:v + 1], aabb=aabb, settle=False, amap=single)
    assert torch.equal(batch.state[:2 * shape[0] * shape[1]], single.state[:2 * shape[0] * shape[1]])
    np.testing.assert_array_equal(batch.read()[2], single.read()[2])
    again = AbiMap(shape)                                                            # the same inputs give the same bytes
    check(shape, rows, align, yaws, locs, centres, aabb=aabb, settle=False, amap=again)
    assert torch.equal(batch.state, again.state)


def test_six_views_of_640_beams_at_98():
    rng = np.random.default_rng(22)
    aabb, locs, centres, rows, yaws = _random_views(rng, (98, 98), 6, 640, 0.1, (0.3, 6.0))
    _, visits, info = check((98, 98), rows, SR.align_angles(640), yaws, locs, centres, aabb=aabb, res=0.1, H=2)
    assert info[3] == 6 * 640 and visits.max() >= 3


def test_one_view_at_the_cap():
    rng = np.random.default_rng(23)
    aabb, locs, centres, rows, yaws = _random_views(rng, (198, 198), 1, 640, 0.05, (0.5, 9.0))
    codes, _, _ = check((198, 198), rows, SR.align_angles(640), yaws, locs, centres, aabb=aabb, res=0.05, H=1)
    assert (codes == 1).sum() > 1000
    aabb, locs, centres, rows, yaws = _random_views(rng, (1, 13331), 2, 6, 0.05, (0.5, 900.0))      # the longest grid the cap admits
    check((1, 13331), rows, SR.align_angles(6), yaws, locs, centres, aabb=aabb, res=0.05)


# ------------------------------------------------------------------ the goal map and the goal pick
def gpu_goal_map(blocked, visits, field=None):
    from apnrf_amd import _lib as L
    from apnrf_amd import planning
    nx, nz = blocked.shape
    n = nx * nz
    vw, vm = _guarded(n, torch.float64, MARKF)
    cw, cells = _guarded(2 * n, torch.int32, MARK32)
    nw, count = _guarded(1, torch.int64, MARK64)
    table = planning._decay_table()
    d = [_dev(np.asarray(blocked, np.int32)), _dev(np.asarray(visits, np.int32)), None if field is None else _dev(np.asarray(field).view(np.int32)),
         _dev(table)]
    L.launch(L.load_library().mnf_planner_goal_map, L.ptr(d[0]), L.ptr(d[1]), L.ptr(d[2]), nx, nz, L.ptr(d[3]), len(table), L.ptr(vm), L.ptr(cells),
             L.ptr(count), device=torch.device(DEV))
    torch.cuda.synchronize()
    _assert_guards(vw, n, MARKF, "vm")
    _assert_guards(cw, 2 * n, MARK32, "cells")
    _assert_guards(nw, 1, MARK64, "count")
    return vm.cpu().numpy().reshape(nx, nz), cells.cpu().numpy().reshape(n, 2), int(count.cpu().numpy()[0])


def _assert_goal_map(blocked, visits, field=None):
    vm, cells, count = gpu_goal_map(blocked, visits, field)
    want_vm = SR.vm_of(blocked, visits)
    want_cells, want_count = SR.padded_goal_list(want_vm, field)
    np.testing.assert_array_equal(vm, want_vm)
    np.testing.assert_array_equal(cells, want_cells)
    assert count == want_count
    np.testing.assert_array_equal(cells[:count], np.argwhere((want_vm >= 0) & (True if field is None else np.asarray(field) != SR.UNREACHED)))
    return vm, cells, count


def _walled_map(shape, seed):
    rng = np.random.default_rng(seed)
    blocked = (rng.random(shape) < 0.15).astype(np.int32)
    blocked[4:9, 3] = blocked[4:9, 8] = blocked[4, 3:9] = blocked[8, 3:9] = 1          # a closed wall around (6, 5)
    blocked[5:8, 4:8] = 0
    visits = rng.integers(0, 40, shape).astype(np.int32)
    return blocked, visits


@pytest.mark.parametrize("shape", [(1, 1), (5, 4), (33, 31), (32, 32), (98, 98), (198, 198)])       # 32 x 32: exactly one full tile of the compaction
def test_goal_map_without_a_field(shape):
    rng = np.random.default_rng(shape[0])
    blocked = (rng.random(shape) < 0.4).astype(np.int32) * rng.integers(1, 3, shape).astype(np.int32)
    visits = rng.integers(3, 60, shape).astype(np.int32)
    _assert_goal_map(blocked, visits)
    if shape == (33, 31):
        visits[5, 7] = 20000                                                         # exp(-m / 5) has long been 0.0
        blocked[5, 7] = 0
        vm, _, _ = _assert_goal_map(blocked, visits)
        assert vm[5, 7] == 0.0
        blocked[2, 2] = -3                                                           # not above 0: free
        assert _assert_goal_map(blocked, visits)[0][2, 2] >= 0


def test_goal_map_of_an_all_blocked_map():
    vm, cells, count = _assert_goal_map(np.ones((7, 9), np.int32), np.arange(63, dtype=np.int32).reshape(7, 9))
    assert count == 0 and (vm == -1).all() and (cells == -1).all()


def test_goal_map_with_a_field():
    from apnrf_amd import planning
    blocked, visits = _walled_map((24, 20), 5)
    free = np.argwhere(blocked == 0)
    outside = tuple(int(v) for v in free[np.argmax((free[:, 0] > 10))])
    for start in (outside, (6, 5)):                                                  # the open floor, and the start enclosed by the wall
        f = planning.path_field(_dev(blocked), [list(start)])["field"][0].cpu().numpy().view(np.uint32)
        _, cells, count = _assert_goal_map(blocked, visits, f)
        inside = {(x, z) for x in range(5, 8) for z in range(4, 8)}
        listed = {tuple(int(v) for v in c) for c in cells[:count]}
        assert (listed == inside) if start == (6, 5) else (count > 12 and not (listed & inside))
    unreached = np.full((24, 20), SR.UNREACHED, np.uint32)
    assert _assert_goal_map(blocked, visits, unreached)[2] == 0


def test_goal_cells_and_draw_goals():
    from apnrf_amd import planning
    blocked, visits = _walled_map((24, 20), 6)
    aabb, res = [0.0, 0.0, 0.0, 24 * 0.2, 20 * 0.2, 1.0], 0.2
    d = planning.Dijkstra(aabb, blocked, res, 0.05, device=DEV)
    b, v = _dev(blocked), _dev(visits)
    for start in (None, (6 * res, 5 * res), (15 * res, 12 * res), (-9.0, 3.0)):
        out = planning.goal_cells(b, v) if start is None else planning.goal_cells(b, v, d, start)
        field = None
        if start is not None:
            f = d._field(*start)
            field = np.full(blocked.shape, SR.UNREACHED, np.uint32) if f is None else f.cpu().numpy().view(np.uint32)
        want_vm = SR.vm_of(blocked, visits)
        want_cells, n = SR.padded_goal_list(want_vm, field)
        np.testing.assert_array_equal(out["vm"].cpu().numpy(), want_vm)
        np.testing.assert_array_equal(out["cells"].cpu().numpy(), want_cells)
        assert out["count"].cpu().numpy().tolist() == [n]
        if start == (-9.0, 3.0):
            assert n == 0
        u = [0.0, np.nextafter(1.0, 0.0), 0.5]
        if n:
            ks = np.array([1, 2, n // 2, n - 1], np.float64)
            u += (ks / n).tolist() + np.nextafter(ks / n, 0.0).tolist() + np.random.default_rng(3).random(50).tolist()
        got = planning.draw_goals(out["cells"], out["count"], u)
        assert got.dtype == torch.int32 and tuple(got.shape) == (len(u), 2)
        np.testing.assert_array_equal(got.cpu().numpy(), SR.pick(want_cells, n, u))
        np.testing.assert_array_equal(planning.draw_goals(out["cells"], out["count"], _dev(np.float64(u))).cpu().numpy(), got.cpu().numpy())
    again = planning.goal_cells(b, v)                                                # the same inputs give the same bytes
    first = planning.goal_cells(b, v)
    assert all(torch.equal(again[k], first[k]) for k in ("vm", "cells", "count"))


def test_scan_cost_map_feeds_the_goal_map(fixture):
    """The visit counts of a ScanCostMap go into goal_cells as they stand: no host copy in between."""
    from apnrf_amd import planning
    c = fixture["small"]
    m = planning.ScanCostMap(c["aabb"], float(c["res"]), device=DEV)
    m.update(c["depth"], c["poses"])
    blocked = (m.codes == 2).to(torch.int32)
    out = planning.goal_cells(blocked, m.visits)
    want_vm = SR.vm_of(blocked.cpu().numpy(), c["visiting"][-1])
    np.testing.assert_array_equal(out["vm"].cpu().numpy(), want_vm)
    np.testing.assert_array_equal(out["cells"].cpu().numpy()[:int(out["count"].item())], np.argwhere(want_vm >= 0))
