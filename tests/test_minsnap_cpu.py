"""The numpy restatement of the min-snap trajectory unit (tests/minsnap_ref.py) against the reference's own answers
(tests/golden/minsnap_trajectories.npz, written by tests/golden/make_golden_minsnap.py), and the unit's place in the header and the binding
table.  No GPU.

What is a chain of separately rounded operations in the reference's order is held to array_equal: delta_t, t_keyframes, yaw_execute, the
sample counts and times, accept / null / reject, the look-around rows.  The coefficients come from another elimination order, so they and what
is evaluated from them are held to bounds that follow from backward stability:
  residual   |A c - b|_inf <= 64 eps (|A|_inf |c|_inf + |b|_inf) =: rho, A assembled by the restatement from the golden's delta_t; asserted
             for the restatement's c and measured for the reference's own c (its dense LU is held to the same rho);
  coeffs     A (c - c_ref) = r - r_ref, so |c - c_ref|_inf <= |A^-1|_inf (rho + rho_ref) =: dc;
  x, yaw     a polynomial in tau <= max delta_t: |dx| <= dc sum_k tau^k; x_ddot likewise with k (k - 1) tau^(k-2);
  rotation   R = [b1 b2 b3] turns with the thrust direction and the yaw: |dR| <= 4 (|d x_ddot| / (9.81 - |x_ddot|_max) + |d yaw|) + 64 eps.
The largest measured deviation per quantity goes to profiles/minsnap_parity.txt with the fixture's cond(A); the GPU test allows the device 8
times those against the golden."""
import ctypes
import os
import re

import numpy as np
import pytest

import minsnap_ref as MR

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = MR.GOLDEN
SYMBOLS = ("mnf_minsnap_workspace_bytes", "mnf_minsnap_solve", "mnf_minsnap_sample_count", "mnf_minsnap_sample_fill")


@pytest.fixture(scope="module")
def golden():
    g = np.load(GOLDEN)
    return g, MR.golden_paths(g)


@pytest.fixture(scope="module")
def restated(golden):
    g, paths = golden
    out = []
    for p in paths:
        pts = MR.waypoints_of_cells(p["cells"], float(g["resolution"]), g["origin"], float(g["height"]))
        out.append(MR.restate(pts))
    return out


def test_header_and_bindings():
    from apnrf_amd import _lib as L
    header = open(os.path.join(REPO, "include", "mi355nerf.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for s in SYMBOLS:
        assert re.search(r"\b" + s + r"\s*\(", code), f"{s} is not declared in include/mi355nerf.h"
        assert s in L.SIGNATURES
    assert L.SIGNATURES["mnf_minsnap_workspace_bytes"][0] is ctypes.c_int64
    assert len(L.SIGNATURES["mnf_minsnap_solve"][1]) == 20 and len(L.SIGNATURES["mnf_minsnap_sample_fill"][1]) == 22
    for name, value in (("MAX_SEGMENTS", 1023), ("OK", 0), ("NULL", 1), ("REJECTED_SHORT", 2), ("SINGULAR", 4), ("TOO_LONG", 8), ("NOT_FINITE", 16),
                        ("SAMPLE_OVERFLOW", 32), ("SAMPLE_INVALID", 64)):
        assert re.search(r"#define\s+MNF_MINSNAP_%s\s+%d\b" % (name, value), code), name
    from apnrf_amd import trajectory as TJ
    assert (TJ.OK, TJ.NULL, TJ.REJECTED_SHORT, TJ.SINGULAR, TJ.TOO_LONG, TJ.NOT_FINITE) == (0, 1, 2, 4, 8, 16)


def test_fixture_holds_its_cases(golden):
    g, paths = golden
    counts = sorted(p["cells"].shape[0] for p in paths)
    for n in (1, 2, 3, 4, 5, 9, 17, 33, 60):
        assert n in counts
    assert counts.count(2) == 2
    acc = [p for p in paths if p["accepted"]]
    assert sum(p["times"].shape[0] == p["N"] + 1 for p in acc) >= 2 and sum(p["times"].shape[0] == p["N"] + 2 for p in acc) >= 2
    assert any(p["cmd_q"][:, 3].min() < 0 < p["cmd_q"][:, 3].max() for p in acc)
    assert max(p["cond"] for p in acc) < 1e7
    assert os.path.getsize(GOLDEN) < 411 * 1024


def test_statuses(golden, restated):
    _, paths = golden
    for p, r in zip(paths, restated):
        assert r["status"] == MR.expected_status(p), p["name"]
        assert r["m"] == p["m"], p["name"]
    by = {p["name"]: r["status"] for p, r in zip(paths, restated)}
    assert by["walk1"] == MR.NULL and by["straight2"] == MR.REJECTED_SHORT and by["diagonal2"] == MR.REJECTED_SHORT
    assert by["repeated_cell"] == MR.SINGULAR and by["repeated_last"] == MR.OK      # a delta_t of 0: the reference's rank test refuses it too


def test_time_allocation_and_sample_times_exact(golden, restated):
    _, paths = golden
    for p, r in zip(paths, restated):
        if not p["accepted"]:
            continue
        for key in ("delta_t", "t_keyframes", "yaw_execute", "times"):
            assert np.array_equal(r[key], p[key]), (p["name"], key)
        assert r["poses"].shape == p["poses"].shape, p["name"]
        S = p["times"].shape[0]
        assert np.array_equal(r["poses"][S:, 3:], p["poses"][S:, 3:]), p["name"]     # the look-around quaternions, signs as scipy leaves them
        assert (r["poses"][S:, :3] == r["poses"][S - 1, :3]).all() and (p["poses"][S:, :3] == p["poses"][S - 1, :3]).all()


def test_parity_with_the_reference(golden, restated):
    _, paths = golden
    worst = {q: 0.0 for q in MR.QUANTITIES}
    lines = []
    for p, r in zip(paths, restated):
        if not p["accepted"]:
            continue
        b = MR.forward_bounds(p)
        res, rho = MR.residual_bound(p["delta_t"], b["keyframes"], r["coeffs"])
        got = {"coeffs": r["coeffs"], "x": r["flat"]["x"], "x_ddot": r["flat"]["x_ddot"], "yaw": r["flat"]["yaw"], "poses": r["poses"]}
        dev = MR.deviations(got, p)
        lines.append(f"restatement {p['name']:>14} m={p['m']:3d} cond={p['cond']:.3e} residual={res:.3e} (reference {b['residual_reference']:.3e}, rho {rho:.3e}) "
                     + " ".join(f"{q}={dev[q]:.3e}" for q in MR.QUANTITIES))
        print(lines[-1])
        for q in MR.QUANTITIES:
            worst[q] = max(worst[q], dev[q])
        assert res <= rho, (p["name"], res, rho)
        for q in MR.QUANTITIES:
            assert dev[q] <= b[q], (p["name"], q, dev[q], b[q])
        # component-wise, sign included, wherever the reference's |w| is away from 0 (there the sign is a rounding accident)
        S = p["times"].shape[0]
        firm = np.abs(p["poses"][:S, 6]) > 1e-9
        assert np.abs(r["poses"][:S, 3:][firm] - p["poses"][:S, 3:][firm]).max() <= b["pose_rotation"], p["name"]
    lines.append("restatement worst " + " ".join(f"{q}={worst[q]:.3e}" for q in MR.QUANTITIES))
    MR.write_parity("restatement", lines)


def test_dense_route_agrees(golden, restated):
    """The timing yardstick solves as the reference does; on a short path it gives the restatement's curve to rounding."""
    g, paths = golden
    k = [p["name"] for p in paths].index("walk9")
    pts = MR.waypoints_of_cells(paths[k]["cells"], float(g["resolution"]), g["origin"], float(g["height"]))
    dense = MR.restate(pts, dense=True)
    assert dense["status"] == MR.OK
    assert np.abs(dense["coeffs"] - paths[k]["coeffs"]).max() <= MR.forward_bounds(paths[k])["coeffs"]
    short = MR.waypoints_of_cells(paths[[p["name"] for p in paths].index("straight2")]["cells"], float(g["resolution"]), g["origin"])
    kept, _, delta_t, tk = MR.time_allocation(short)
    assert delta_t[0] > 3999.0                                                        # 2 d / 1e-4: what the rule for two waypoints rests on
    keyframes = np.concatenate([kept, MR.yaw_execute(tk, 2 * np.pi, 0.0)[:, None]], axis=1)
    assert MR.solve(delta_t, keyframes, dense=True) is None                           # the reference's rank test refuses it


def test_look_table_matches_scipy():
    from scipy.spatial.transform import Rotation
    want = np.array([Rotation.from_euler("y", a, degrees=True).as_quat() for a in np.linspace(0, 360, 20)])
    assert np.array_equal(MR.look_quats(), want)
    from apnrf_amd import trajectory as TJ
    assert np.array_equal(TJ.look_quaternions(np.linspace(0, 360, 20)), want)
