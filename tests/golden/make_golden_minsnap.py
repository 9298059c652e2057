"""Writes tests/golden/minsnap_trajectories.npz: the reference's own curves, samples and view poses for a dozen grid paths.

    python tests/golden/make_golden_minsnap.py --reference /path/to/the/reference/tree

The reference's MinSnap (planning/rotorpy/rotorpy/trajectories/minsnap.py), SE3Control.update_ref (controllers/quadrotor_control.py), time_exit,
merge_dicts and the two sanitize functions (rotorpy/simulate.py) are imported at generation time only and driven the way sample_traj drives
them (planning/planning_funcs.py:328-397): the path reversed, index * resolution + aabb[:3] with the height 1.7, yaw = linspace(2 pi, 0, n),
v_avg = 0.5, 20 samples a second and at least 20, the axis shuffle of cmd_q through scipy's rotation vectors, 20 look-around poses.  What the
reference imports and this container lacks (cvxopt: MinSnap never calls it) is placeholdered, as make_golden_clearance.py does.  The fixture
holds data only.  Paths are 8-connected cell lists at 0.2 m in the order mnf_path_trace lists them, goal first.  The generator asserts, on the
reference's answers alone, that the fixture holds each kind of case the tests rely on."""
import argparse
import contextlib
import io
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

RESOLUTION = 0.2
ORIGIN = np.array([-2.4, -3.0, -0.3])          # aabb[:3]
HEIGHT = 1.7
LENGTHS = (1, 2, 2, 3, 4, 5, 9, 17, 33, 60)
MOVES = [(1, 0), (0, 1), (-1, 0), (0, -1), (-1, -1), (-1, 1), (1, -1), (1, 1)]


class _Anything(types.ModuleType):
    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return lambda *a, **k: None


def _placeholder(name):
    try:
        __import__(name)
    except Exception:
        parts = name.split(".")
        for i in range(1, len(parts) + 1):
            sys.modules.setdefault(".".join(parts[:i]), _Anything(".".join(parts[:i])))


def import_reference(root):
    sys.path.insert(0, os.path.join(root, "planning", "rotorpy"))
    _placeholder("cvxopt")
    from rotorpy.controllers.quadrotor_control import SE3Control
    from rotorpy.simulate import merge_dicts, sanitize_control_dic, sanitize_trajectory_dic, time_exit
    from rotorpy.trajectories.minsnap import MinSnap
    from rotorpy.vehicles.crazyflie_params import quad_params
    return types.SimpleNamespace(SE3Control=SE3Control, MinSnap=MinSnap, merge_dicts=merge_dicts, sanitize_control_dic=sanitize_control_dic,
                                 sanitize_trajectory_dic=sanitize_trajectory_dic, time_exit=time_exit, quad_params=quad_params)


def walk(rng, n, straightness=0.6):
    """An 8-connected path of n cells that never steps back onto the cell it came from, start first."""
    cells = [(int(rng.integers(20, 40)), int(rng.integers(20, 40)))]
    move = MOVES[int(rng.integers(8))]
    while len(cells) < n:
        if rng.uniform() > straightness:
            move = MOVES[int(rng.integers(8))]
        nxt = (cells[-1][0] + move[0], cells[-1][1] + move[1])
        if len(cells) >= 2 and nxt == cells[-2] or min(nxt) < 0:
            move = MOVES[int(rng.integers(8))]
            continue
        cells.append(nxt)
    return cells


def make_paths(rng):
    """-> (names, cell lists start first)."""
    names, paths = [], []
    for n in LENGTHS:
        p = walk(rng, n)
        if n == 2:
            first = "straight2" not in names
            p = [p[0], (p[0][0] + 1, p[0][1])] if first else [p[0], (p[0][0] + 1, p[0][1] - 1)]
            names.append("straight2" if first else "diagonal2")
        else:
            names.append(f"walk{n}")
        paths.append(p)
    p = walk(rng, 12)
    names.append("repeated_cell")
    paths.append(p[:5] + [p[4]] + p[5:])                          # a cell twice in a row: seg_mask drops a waypoint, but the time allocation
                                                                  # indexes the UNMASKED distances, so a delta_t is 0 and the reference refuses
    p = walk(rng, 10)
    names.append("repeated_last")
    paths.append(p + [p[-1]])                                     # the goal twice: the zero distance lies past the m the recurrence reads
    return names, paths


def drive(ref, controller, cells_start_first):
    """sample_traj's inner block for one path -> a dict of the reference's answers."""
    from scipy.spatial.transform import Rotation
    aabb = np.concatenate([ORIGIN, ORIGIN + 12.8])
    xs = [c[0] * RESOLUTION + 0 for c in cells_start_first]      # Dijkstra.calc_position: index * resolution + min, min = 0
    ys = [c[1] * RESOLUTION + 0 for c in cells_start_first]
    dij_waypoints = np.array([xs, ys, np.linspace(HEIGHT, HEIGHT, len(xs))]).T + aabb[:3]
    yaw = np.linspace(2 * np.pi, 0, len(dij_waypoints))
    trajectory = ref.MinSnap(points=dij_waypoints, yaw_angles=yaw, v_avg=0.5)
    with contextlib.redirect_stdout(io.StringIO()):
        initialized = bool(trajectory.initialize())
    out = {"initialized": initialized, "null": bool(trajectory.null), "m": int(trajectory.m), "waypoints": dij_waypoints}
    if trajectory.m >= 1 and hasattr(trajectory, "delta_t"):
        out["delta_t_refused"] = np.array(trajectory.delta_t)
    if not initialized or trajectory.null:
        return out
    t_final = np.sum(trajectory.delta_t)
    n_steps = max(int(t_final * 20), 20)
    t_step = t_final / n_steps
    times, flats, commands = [0], [], []
    while True:                                                   # a sample at 0, then one per step until time_exit speaks
        flats.append(ref.sanitize_trajectory_dic(trajectory.update(times[-1])))
        commands.append(ref.sanitize_control_dic(controller.update_ref(times[-1], flats[-1])))
        if ref.time_exit(times[-1], t_final):
            break
        times.append(times[-1] + t_step)
    time = np.array(times, dtype=float)
    flat = ref.merge_dicts(flats)
    cmd_q = ref.merge_dicts(commands)["cmd_q"]
    position = flat["x"][:, [0, 2, 1]]                            # x, z, y
    shuffled = np.empty_like(cmd_q)
    for k, q in enumerate(cmd_q):                                 # one rotation at a time, as the reference converts them
        rv = Rotation.from_quat(q).as_rotvec()
        shuffled[k] = Rotation.from_rotvec(np.array([-rv[0], rv[2], -rv[1]])).as_quat()
    rows = [np.hstack((position, shuffled))]
    for angle in np.linspace(0, 360, 20):
        rows.append(np.concatenate([position[-1], Rotation.from_euler("y", angle, degrees=True).as_quat()])[None])
    traj_x_quat = np.vstack(rows)
    N_sample_disc = n_steps
    m = trajectory.m
    c_opt = np.empty((m, 4, 8))
    c_opt[:, :3] = trajectory.x_poly[:, :, ::-1]                  # x_poly is flip(c_opt): back to the lowest power first
    c_opt[:, 3] = trajectory.yaw_poly[:, 0, ::-1]
    import importlib
    MS = importlib.import_module(ref.MinSnap.__module__)
    A = MS.get_1d_equality_constraints(trajectory.points[:, 0], trajectory.delta_t, m)[0]
    out.update(delta_t=np.array(trajectory.delta_t), t_keyframes=np.array(trajectory.t_keyframes), yaw_execute=np.array(trajectory.yaw_execute), c_opt=c_opt,
               times=time, x=flat["x"], x_ddot=flat["x_ddot"], yaw=flat["yaw"], cmd_q=cmd_q, poses=traj_x_quat, N=N_sample_disc, cond=float(np.linalg.cond(A)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="the reference tree (planning/rotorpy)")
    ap.add_argument("--out", default=os.path.join(HERE, "minsnap_trajectories.npz"))
    args = ap.parse_args()
    ref = import_reference(args.reference)
    controller = ref.SE3Control(ref.quad_params)
    rng = np.random.default_rng(41)
    names, paths = make_paths(rng)
    answers = [drive(ref, controller, p) for p in paths]
    # both kinds of sample count, on the reference's answers alone: draw further short walks until each kind is there twice
    def kinds():
        acc = [a for a in answers if a["initialized"] and not a["null"]]
        return sum(a["times"].shape[0] == a["N"] + 1 for a in acc), sum(a["times"].shape[0] == a["N"] + 2 for a in acc)
    while min(kinds()) < 2 and len(paths) < 17:
        p = walk(rng, int(rng.integers(6, 14)))
        a = drive(ref, controller, p)
        short = 0 if kinds()[0] < 2 else 1
        if a["initialized"] and a["times"].shape[0] == a["N"] + 1 + short:
            names.append(f"extra{len(p)}")
            paths.append(p)
            answers.append(a)
    n = len(paths)
    accepted = np.array([a["initialized"] and not a["null"] for a in answers])
    acc = [a for a in answers if a["initialized"] and not a["null"]]

    # the fixture's conditions
    assert 12 <= n <= 17, n
    plus1, plus2 = kinds()
    assert plus1 >= 2 and plus2 >= 2, (plus1, plus2)
    by_name = dict(zip(names, answers))
    assert by_name["walk1"]["null"] and by_name["walk1"]["initialized"] and not accepted[names.index("walk1")]
    for two in ("straight2", "diagonal2"):
        assert not by_name[two]["initialized"] and not by_name[two]["null"] and by_name[two]["m"] == 1, two
        assert by_name[two]["delta_t_refused"][0] > 3999.0, by_name[two]["delta_t_refused"]
    for k, a in enumerate(answers):
        if len(paths[k]) >= 3 and names[k] != "repeated_cell":
            assert accepted[k], names[k]
    rep = by_name["repeated_cell"]
    assert rep["m"] == len(paths[names.index("repeated_cell")]) - 2 and not rep["initialized"] and not rep["null"]
    assert (rep["delta_t_refused"] == 0).sum() == 1
    assert by_name["repeated_last"]["m"] == len(paths[names.index("repeated_last")]) - 2 and accepted[names.index("repeated_last")]
    assert sorted(a["m"] for a in acc)[:4] == [2, 3, 4, 8] or {2, 3, 4, 8} <= {a["m"] for a in acc}
    assert max(a["m"] for a in acc) == 59
    w = [a["cmd_q"][:, 3] for a in acc]
    assert any((v.min() < 0 < v.max()) and np.abs(v).min() < 0.05 for v in w), "no yaw sweep passes w = 0"
    assert max(a["cond"] for a in acc) < 1e7, max(a["cond"] for a in acc)
    assert all(np.abs(a["x_ddot"]).max() < 9.0 for a in acc), [float(np.abs(a["x_ddot"]).max()) for a in acc]   # the thrust axis stays well away from 0

    def packed(key, items):
        off = np.zeros(len(items) + 1, np.int64)
        off[1:] = np.cumsum([0 if v is None else v.shape[0] for v in items])
        rows = [v for v in items if v is not None and v.shape[0]]
        return off, np.concatenate(rows)

    def field(key):
        return [a[key] if ok else None for a, ok in zip(answers, accepted)]

    cell_offsets, cells = packed("cells", [np.array(p[::-1], np.int32) for p in paths])          # goal first, as a trace lists them
    seg_offsets, delta_t = packed("delta_t", field("delta_t"))
    _, c_opt = packed("c_opt", field("c_opt"))
    key_offsets, t_keyframes = packed("t_keyframes", field("t_keyframes"))
    _, yaw_execute = packed("yaw_execute", field("yaw_execute"))
    sample_offsets, times = packed("times", field("times"))
    _, x = packed("x", field("x"))
    _, x_ddot = packed("x_ddot", field("x_ddot"))
    _, yaw = packed("yaw", field("yaw"))
    _, cmd_q = packed("cmd_q", field("cmd_q"))
    pose_offsets, poses = packed("poses", field("poses"))
    np.savez_compressed(args.out, n_paths=np.int64(n), names=np.array(names), resolution=np.float64(RESOLUTION), origin=ORIGIN, height=np.float64(HEIGHT),
                        cells=cells, cell_offsets=cell_offsets, initialized=np.array([a["initialized"] for a in answers]),
                        null=np.array([a["null"] for a in answers]), accepted=accepted, m=np.array([a["m"] for a in answers], np.int32),
                        N=np.array([a.get("N", 0) for a in answers], np.int64), cond=np.array([a.get("cond", 0.0) for a in answers]),
                        seg_offsets=seg_offsets, delta_t=delta_t, c_opt=c_opt, key_offsets=key_offsets, t_keyframes=t_keyframes, yaw_execute=yaw_execute,
                        sample_offsets=sample_offsets, times=times, x=x, x_ddot=x_ddot, yaw=yaw, cmd_q=cmd_q, pose_offsets=pose_offsets, poses=poses)
    size = os.path.getsize(args.out)
    assert size < 411 * 1024, size
    print(f"{n} paths ({', '.join(names)}), {int(accepted.sum())} accepted, {plus1} with N + 1 samples and {plus2} with N + 2, {times.shape[0]} samples, "
          f"cond(A) up to {max(a['cond'] for a in acc):.3g}")
    print("wrote", args.out, size, "bytes")


if __name__ == "__main__":
    main()
