"""The reference's active-mapping loop (scripts/pipeline.py:1025-1224) at small sizes, from public calls only, with the scene sensor in the
place of habitat_sim: a closed procedural room, 64 x 64 captures, one field, a 2^14 hash table.

  1. the initial yaw sweep at the start pose -> `Dataset.update_data` (device tensors) and `ScanCostMap.update`;
  2. training on it;
  3. per planning step: the planner's map from the estimator, `goal_cells` + `draw_goals`, `candidate_trajectories` (grid search, min-snap
     curves, samples, view poses) with `trajectory_clearance`, `score_views` per candidate and the argmax, captures along the winner,
     `update_data` and `ScanCostMap.update`, `train_step`s, `evaluate_views` on held-out captures.

With `--pose-noise DEG,CM` every capture of a planning step arrives with a drifted pose (a rotation of DEG degrees about a random axis, CM centimetres
along a random direction) and is relocalised against the current field before it is trained on (`localize.PoseRefiner`, all views of the step in one batch);
the step's line then carries the mean pose error before and after.  The initial sweep keeps its poses: there is no map to relocalise against yet.

With `--tsdf` every batch of captures is also fused into a `tsdf.TsdfVolume` at the world's 10 cm (from the dataset's own storage and poses), and each
step's line gains the observed fraction of its lattice, the triangle count of its mesh, and the accuracy and completion of the field's mesh
(`extract_surface` at iso = occ_thre / render_step_size) against points sampled from the TSDF mesh every 5 cm.  Without the flag every line stays as it is.

One line per planning step.  The whole run is one child process under `timeout`; the driver starts no GPU work itself.  Nothing here is a
measurement of speed and nothing is asserted: it shows the stages joined end to end on the device.

    python tools/active_loop.py [--steps 3] [--out profiles/active_loop.txt]
    python tools/active_loop.py --pose-noise 1,3 --out profiles/active_loop_pose_noise.txt
    python tools/active_loop.py --tsdf --out profiles/active_loop_tsdf.txt
"""
import argparse
import os
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

DEV = "cuda:0"
AABB = np.array([-4.0, -0.2, -4.0, 4.0, 2.2, 4.0])                                      # x, y, z: 40 x 12 x 40 cells of 0.2 m, walls every 4 m with doors
CELL, SIDE = 0.2, 64
START = np.array([-2.0, 1.0, -2.0])
KW = dict(near_plane=0.1, render_step_size=5e-3, cone_angle=0.004, alpha_thre=0.01)


def pose_errors(c2w, truth):
    """(mean rotation error in degrees, mean translation error in cm) of poses [n,4,4] against `truth`"""
    c2w, truth = np.asarray(c2w, np.float64), np.asarray(truth, np.float64)
    rel = np.einsum("nij,nkj->nik", c2w[:, :3, :3], truth[:, :3, :3])
    ang = np.degrees(np.arccos(np.clip((np.trace(rel, axis1=1, axis2=2) - 1.0) / 2.0, -1.0, 1.0)))
    return float(ang.mean()), float(100.0 * np.linalg.norm(c2w[:, :3, 3] - truth[:, :3, 3], axis=1).mean())


def run(steps, train_steps, n_goals, seed, pose_noise=None, refine_iters=40, tsdf=False):
    import torch
    from apnrf_amd import localize as LZ
    from apnrf_amd import clearance as CL
    from apnrf_amd import nerfacc as NA
    from apnrf_amd import planning as PL
    from apnrf_amd import render as RD
    from apnrf_amd import sensor as SN
    from apnrf_amd import synthetic as S
    from apnrf_amd.dataset import Dataset, planner_path_finding_map
    from apnrf_amd.ngp import NGPRadianceField
    from apnrf_amd.optim import FusedAdam
    from apnrf_amd.trajectory import candidate_trajectories
    rng = np.random.default_rng(seed)
    torch.manual_seed(seed)
    res = [int(round((AABB[3 + k] - AABB[k]) / CELL)) for k in range(3)]
    occ = S.make_occupancy(res, seed=seed, clutter=0.01, aabb=AABB, free_at=[START])
    world = SN.VoxelScene.from_occupancy(occ, AABB, cell=CELL, refine=2, closed=True, device=DEV)
    sim = SN.VoxelSim(world, SIDE, SIDE)
    aabb_xzy = AABB[[0, 2, 1, 3, 5, 4]]
    aabb32 = torch.from_numpy(AABB.astype(np.float32))
    field = NGPRadianceField(aabb=aabb32, neurons=128, layers=2, num_semantic_classes=29, log2_hashmap_size=14, seed=seed).to(DEV)
    est = NA.OccGridEstimator(aabb32, resolution=res, levels=1).to(DEV)
    opt = FusedAdam(field.parameters(), lr=2e-3, eps=1e-15).bind_field(field)
    data = Dataset(training=True, save_fp="", num_rays=1024, device=DEV)
    cost = PL.ScanCostMap(AABB, CELL, device=DEV)
    fused = None
    if tsdf:
        from apnrf_amd import cloud as CD
        from apnrf_amd import surface as SF
        from apnrf_amd.tsdf import TsdfVolume
        fused = TsdfVolume(AABB, world.voxel_size, device=DEV)

    def tsdf_report():
        """The classical map beside the neural one: the field's mesh against points on the TSDF mesh."""
        counts = fused.counts()
        classical = fused.extract_mesh()
        text = f"; tsdf {100.0 * counts['observed_fraction']:.1f} % observed, {classical.n_triangles} triangles"
        neural = SF.extract_surface(field.eval(), est.eval(), 1e-2 / KW["render_step_size"])
        if classical.n_triangles == 0 or neural.n_triangles == 0:
            return text + f", field mesh {neural.n_triangles} triangles: nothing to compare"
        points = CD.sample_mesh_points(classical, resolution=0.05)[0]
        q = CD.mesh_quality(neural, points, resolution=0.05, threshold=0.1, r_max=0.5)
        return text + f", field mesh {neural.n_triangles} triangles: accuracy {q['accuracy']:.3f} m, completion {q['completion']:.3f} m against the tsdf mesh"
    c2w_of = lambda poses: torch.from_numpy(np.stack([RD.pose_to_c2w(p) for p in np.asarray(poses, np.float64).reshape(-1, 7)])).to(DEV)

    noise_rng = np.random.default_rng(seed + 1)      # (its own stream: the loop's draws are the same with and without the leg)

    def capture(poses, drift=None):
        """What the reference does with a batch of captures: the dataset takes colour, depth (along the ray, what the field renders) and
        classes; the cost map takes the planar depth's middle rows.  `drift` (degrees, cm): the poses arrive perturbed and are refined
        against the current field before anything trains on them -> the pose errors before and after."""
        c2w = c2w_of(poses)
        rgba, depth_ray, sem = sim.sample_images_from_poses(poses, depth="ray")
        planar = sim.sample_images_from_poses(poses)[1]
        report = None
        if drift is not None:
            truth = c2w.cpu().numpy()
            n = truth.shape[0]
            axes, dirs = noise_rng.standard_normal((n, 3)), noise_rng.standard_normal((n, 3))
            axes, dirs = axes / np.linalg.norm(axes, axis=1, keepdims=True), dirs / np.linalg.norm(dirs, axis=1, keepdims=True)
            noisy = LZ.compose_c2w(truth, np.concatenate([axes * np.deg2rad(drift[0]), dirs * drift[1] * 1e-2], 1))
            first = len(data)
            data.update_data(rgba[..., :3], depth_ray, sem, torch.from_numpy(noisy).to(DEV))
            ids = list(range(first, first + n))
            out = LZ.refine_poses(field, est, data, ids, n_iters=refine_iters, rays_per_view=1024, lr_rot=1e-3, lr_trans=2e-3, seed=seed, **KW)
            data.set_camtoworlds(ids, out["c2w"])
            c2w = torch.from_numpy(out["c2w"]).to(DEV)
            report = pose_errors(noisy, truth) + pose_errors(out["c2w"], truth) + (int(out["stalled"].max()), out["status"])
        else:
            data.update_data(rgba[..., :3], depth_ray, sem, c2w)
        if fused is not None:
            fused.integrate_dataset(data, list(range(len(data) - int(c2w.shape[0]), len(data))), depth_along="ray")
        cost.update(planar, c2w)
        return report

    done = [0]

    def train(n):
        for _ in range(n):
            b = data[0]
            RD.train_step(field, est, opt, b["rays"], b["pixels"], b["dep"], b["sem"], b["color_bkgd"], step=done[0], occ_thre=1e-2, deterministic=True, **KW)
            done[0] += 1

    # held-out views: a sweep at another place of the start room
    held = Dataset(training=False, save_fp="", device=DEV)
    hp = S.camera_poses(START + [0.6, 0.0, 0.5], 4)
    hr, hd, hs = sim.sample_images_from_poses(hp, depth="ray")
    held.update_data(hr[..., :3], hd, hs, c2w_of(hp))
    # 1. + 2.
    capture(S.camera_poses(START, 12))
    train(train_steps)
    ev = RD.evaluate_views(field.eval(), est.eval(), held, [0, 1, 2, 3], **KW)["mean"]
    print(f"sweep      12 views, {done[0]} train steps: held-out PSNR {ev['psnr']:.2f}, depth MSE {ev['depth_mse']:.4f}; cost map {cost.info()}", flush=True)
    current = START.copy()
    focal = sim.focal
    for step in range(steps):
        state_xzy = current[[0, 2, 1]]
        blocked = planner_path_finding_map([est], state_xzy, aabb_xzy, CELL, y_slice=int((current[1] - AABB[1]) / CELL))
        cx, cz = int((current[0] - AABB[0]) / CELL), int((current[2] - AABB[2]) / CELL)
        blocked[max(cx - 1, 0):cx + 2, max(cz - 1, 0):cz + 2] = 0                         # the vehicle stands in free space, whatever the field believes so far
        dij = PL.Dijkstra(aabb_xzy, blocked, CELL, 0.1, device=DEV)
        start_xy = (float(current[0] - AABB[0]), float(current[2] - AABB[2]))
        gc = PL.goal_cells(dij.blocked, cost.visits, dij, start_xy)
        goals = PL.draw_goals(gc["cells"], gc["count"], rng.random(n_goals)).cpu().numpy()
        goals = goals[(goals >= 0).all(axis=1)]
        if goals.shape[0] == 0:
            print(f"step {step}     no free cell is reached from the current pose on the estimator's map: nothing to plan", flush=True)
            break
        clear = CL.clearance_field([est], voxel=CELL)
        cand = candidate_trajectories(dij, start_xy, [(float(g[0]) * CELL, float(g[1]) * CELL) for g in goals], aabb_xzy, height=float(current[1] - AABB[1]),
                                      clearance=clear, radius=0.1, host=True)
        if not cand["trajectories"]:
            print(f"step {step}     every one of the {goals.shape[0]} goals was refused (status {cand['curves'].status.tolist()})", flush=True)
            break
        certified = cand["certified"].cpu().numpy()
        scores = []
        for traj in cand["trajectories"]:
            views = traj[np.linspace(0, len(traj) - 1, 6).astype(int)]
            scores.append(float(RD.score_views([field.eval()], [est.eval()], views, SIDE, SIDE, focal, KW["near_plane"], KW["render_step_size"], 0.25, KW["cone_angle"],
                                               KW["alpha_thre"], device=DEV, group=False)[1]))
        best = int(np.argmax(scores))
        traj = cand["trajectories"][best]
        views = traj[np.linspace(0, len(traj) - 1, 6).astype(int)]
        report = capture(views, pose_noise)
        current = views[-1][:3].copy()
        train(train_steps // 2)
        ev = RD.evaluate_views(field.eval(), est.eval(), held, [0, 1, 2, 3], **KW)["mean"]
        print(f"step {step}     {goals.shape[0]} goals, {len(cand['trajectories'])} curves ({int(certified.sum())} certified at 0.1 m), scores "
              f"{min(scores):.3f} .. {max(scores):.3f}, flew curve {cand['kept'][best]} of {len(traj)} poses to ({current[0]:.2f}, {current[1]:.2f}, {current[2]:.2f}); "
              f"{len(data)} views, {done[0]} train steps: held-out PSNR {ev['psnr']:.2f}, depth MSE {ev['depth_mse']:.4f}; sensor misses {int(sim.info[0])}"
              + ("" if report is None else f"; pose error of the {len(views)} captures {report[0]:.2f} deg, {report[1]:.2f} cm -> {report[2]:.2f} deg, {report[3]:.2f} cm after "
                 f"{refine_iters} iterations (stalled at most {report[4]}, status {report[5]})") + (tsdf_report() if fused is not None else ""), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--train-steps", type=int, default=200)
    ap.add_argument("--goals", type=int, default=6)
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--pose-noise", default=None, metavar="DEG,CM", help="perturb the pose of every capture of a planning step and refine it against the field first")
    ap.add_argument("--tsdf", action="store_true", help="fuse every batch of captures into a TSDF volume too and compare the field's mesh with its mesh")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true", help="(internal) run the loop in this process")
    a = ap.parse_args()
    if a.child:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("active_loop needs a GPU")
        import apnrf_amd  # noqa: F401
        run(a.steps, a.train_steps, a.goals, a.seed, tuple(float(x) for x in a.pose_noise.split(",")) if a.pose_noise else None, tsdf=a.tsdf)
        return
    r = subprocess.run(["timeout", "-k", "10", "420", sys.executable, os.path.abspath(__file__), "--child", "--steps", str(a.steps), "--train-steps", str(a.train_steps),
                        "--goals", str(a.goals), "--seed", str(a.seed)] + (["--pose-noise", a.pose_noise] if a.pose_noise else []) + (["--tsdf"] if a.tsdf else []), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    body = [ln for ln in r.stdout.splitlines() if ln.strip() and "amdgpu.ids" not in ln]
    head = (f"# the active-mapping loop at small sizes: a closed {AABB[3] - AABB[0]:.0f} x {AABB[4] - AABB[1]:.1f} x {AABB[5] - AABB[2]:.0f} m procedural world at 10 cm voxels, "
            f"{SIDE} x {SIDE} captures, one 128 x 2 field with a 2^14 table; {a.steps} planning steps, seed {a.seed}"
            + (f"; captures arrive with {a.pose_noise} (deg, cm) of pose noise and are relocalised first" if a.pose_noise else "")
            + ("; every batch of captures is also fused into a TSDF volume at 10 cm (trunc 40 cm, nearest pixel)" if a.tsdf else ""))
    text = "\n".join([head] + (body if r.returncode == 0 else body[-25:] + [f"# the loop ended with status {r.returncode}"]))
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    if r.returncode != 0:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
