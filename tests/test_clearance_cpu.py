"""CPU checks of the numpy restatement tests/clearance_ref.py, which the GPU tests compare the device with: its voxel walk, its floor
division and its collision check against the reference's own answers (tests/golden/clearance_walks.npz, written by
tests/golden/make_golden_clearance.py), and its brute-force distance field against scipy's Euclidean distance transform."""
import numpy as np
import pytest

import clearance_ref as CR


@pytest.fixture(scope="module")
def walks(golden):
    g = golden("clearance_walks")
    return {k: g[k] for k in g.files}


def test_fixture_holds_every_kind_of_chord(walks):
    kinds = [str(k) for k in walks["kinds"]]
    assert kinds == ["octant", "axis", "zero", "same_voxel", "faces", "leaving", "frames"]
    for k in range(len(kinds)):
        assert (walks["kind"] == k).sum() >= 6, kinds[k]
    n = walks["start"].shape[0]
    assert 180 <= n and walks["offsets"].shape == (n + 1,) and walks["offsets"][-1] == walks["voxels"].shape[0]
    assert (walks["origin"][walks["kind"] == kinds.index("frames")] != 0).all()
    assert walks["checker"].any() and (~walks["checker"]).any()
    shape = walks["shape"]
    assert ((walks["voxels"] < 0) | (walks["voxels"] >= shape)).any()                  # a walk that leaves the grid


def test_walk_restatement_equals_the_reference(walks):
    n = walks["start"].shape[0]
    size = float(walks["size"])
    done = 0
    for i in range(n):
        want = walks["voxels"][walks["offsets"][i]:walks["offsets"][i + 1]]
        got, cut, finite = CR.voxel_walk(walks["start"][i], walks["end"][i], walks["current_voxel"][i], walks["end_voxel"][i], size)
        assert finite and not cut
        np.testing.assert_array_equal(got, want, err_msg=f"chord {i}")
        done += 1
    assert done == n                                                                  # no case skipped


def test_the_listed_quirks_are_in_the_fixture(walks):
    kinds = [str(k) for k in walks["kinds"]]
    off, vox = walks["offsets"], walks["voxels"]
    for i in np.flatnonzero(walks["kind"] == kinds.index("zero")):
        assert vox[off[i]:off[i + 1]].tolist() == [(walks["current_voxel"][i] + [0, 0, 1]).tolist()]       # one step in +z
    i = int(np.flatnonzero(walks["kind"] == kinds.index("leaving"))[0])
    np.testing.assert_array_equal(walks["start"][i], [0.9, 0.5, 0.1])
    assert vox[off[i + 1] - 1].tolist() == [-1, 0, 0]                                  # overshoots the end voxel, out of the grid
    for i in range(walks["start"].shape[0]):
        assert not (vox[off[i]:off[i + 1]] == walks["current_voxel"][i]).all(axis=1).any()                 # the start voxel is not listed


def test_floor_divide_restatement_equals_numpy_and_the_reference(walks):
    size = float(walks["size"])
    got = CR.world2voxels(walks["pinned"], size)
    np.testing.assert_array_equal(got, walks["pinned_cells"])
    assert (walks["pinned_cells"] != np.floor(walks["pinned"] / size)).any()           # `//` is not floor(x / size)
    assert CR.floor_divide(1.0, 0.2) == 4.0
    # the voxels the reference derived for the chords
    for key, pos in (("current_voxel", "start"), ("end_voxel", "end")):
        np.testing.assert_array_equal(CR.cells_of_points(walks[pos], [0, 0, 0], size)[walks["origin"].sum(axis=1) == 0],
                                      walks[key][walks["origin"].sum(axis=1) == 0])
        rel = walks[pos] - walks["origin"]
        np.testing.assert_array_equal(CR.world2voxels(rel, size), walks[key])
    # numpy itself, on values of every magnitude and sign, and other divisors
    rng = np.random.default_rng(3)
    a = np.concatenate([rng.uniform(-50, 50, 4000), rng.uniform(-1, 1, 2000) * 10.0 ** rng.integers(-12, 12, 2000), np.arange(-60, 60) * 0.1,
                        [0.0, -0.0, 1e300, -1e300, 5e-324]])
    for b in (0.2, 0.1, 0.05, 0.3, 1.0, 0.07):
        want = a // b
        got = np.array([CR.floor_divide(v, b) for v in a])
        np.testing.assert_array_equal(got, want)
        assert (np.signbit(got) == np.signbit(want)).all()
    with np.errstate(invalid="ignore"):
        for v in (np.inf, -np.inf, np.nan):
            assert np.isnan(CR.floor_divide(v, 0.2)) and np.isnan(np.float64(v) // 0.2)
    assert CR.cell_of(float("nan")) == CR.INT32_MIN and CR.cell_of(1e300) == CR.CELL_FAR and CR.cell_of(-1e300) == -CR.CELL_FAR


def test_collision_checker_restatement_equals_the_reference(walks):
    size = float(walks["size"])
    shape = walks["shape"]
    for i in range(walks["start"].shape[0]):
        aabb = np.concatenate([walks["origin"][i], walks["origin"][i] + shape * size])
        x = np.stack([walks["start"][i], 0.5 * (walks["start"][i] + walks["end"][i]), walks["end"][i]])
        assert CR.collision_checker(walks["grid"], x, size, aabb) == bool(walks["checker"][i]), i


def test_bounded_and_non_finite_walks():
    got, cut, finite = CR.voxel_walk([0.1, 0.1, 0.1], [5.1, 3.1, 0.1], [0, 0, 0], [25, 15, 0], 0.2, max_steps=7)
    assert cut and finite and got.shape == (7, 3)
    got, cut, finite = CR.voxel_walk([0.1, np.nan, 0.1], [5.1, 3.1, 0.1], [0, 0, 0], [25, 15, 0], 0.2)
    assert not finite and not cut and got.shape == (0, 3)


def _grids():
    rng = np.random.default_rng(7)
    a = (rng.uniform(size=(2, 9, 7, 11)) < 0.03).astype(np.uint8)
    b = np.zeros((1, 6, 5, 4), np.uint8)
    b[0, 5, 4, 3] = 1
    c = np.ones((1, 4, 5, 6), np.uint8)
    c[0, 1, 2, 3] = 0
    return a, b, c


def test_brute_force_field_equals_scipy():
    ndimage = pytest.importorskip("scipy.ndimage")
    for g in _grids():
        d2, info = CR.brute_d2(g)
        occ = (g != 0).any(axis=0)
        want = np.rint(ndimage.distance_transform_edt(~occ) ** 2).astype(np.int32)
        np.testing.assert_array_equal(d2, want)
        assert info.tolist() == [int(occ.sum()), int(want.max())]


def test_brute_force_field_known_answers():
    d2, info = CR.brute_d2(np.zeros((1, 3, 4, 5), np.uint8))
    assert (d2 == CR.INT32_MAX).all() and info.tolist() == [0, -1]
    g = np.zeros((1, 3, 4, 5), np.uint8)
    g[0, 0, 0, 0] = 1
    d2, info = CR.brute_d2(g)
    assert d2[2, 3, 4] == 4 + 9 + 16 and d2[0, 0, 0] == 0 and info.tolist() == [1, 29]
    d2, info = CR.brute_d2(np.ones((1, 1, 1, 1), np.uint8))
    assert d2.tolist() == [[[0]]] and info.tolist() == [1, 0]


def test_lookup_restatement_ties_and_outside():
    g = np.zeros((1, 4, 4, 4), np.uint8)
    g[0, 0, 0, 0] = 1
    d2, _ = CR.brute_d2(g)
    pts = np.array([[0.5, 0.5, 0.3], [0.3, 0.5, 0.5], [0.5, 0.3, 0.5], [9.0, 0.1, 0.1], [np.nan, 0.1, 0.1], [0.1, 0.1, 0.1]])
    cells, pd2, traj, info = CR.lookup(d2, [0, 0, 0], 0.2, pts, [0, 3, 3, 5, 6])
    assert pd2.tolist() == [9, 9, 9, -1, -1, 0]                                        # cells (2,2,1), (1,2,2), (2,1,2): all 9
    assert traj.tolist() == [[9, 0, 0, 3], [-1, -1, 0, 0], [-1, -1, 2, 2], [0, 0, 0, 1]]
    assert info.tolist() == [2, 1] and cells[4, 0] == CR.INT32_MIN


def test_d2_threshold():
    assert CR.d2_threshold(0.0, 0.2) == 0 and CR.d2_threshold(0.2, 0.2) == 3 and CR.d2_threshold(0.5, 0.2) == 11
