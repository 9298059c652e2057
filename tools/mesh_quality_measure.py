"""Measurement of the mesh-quality route (DESIGN.md "Mesh quality", profiles/mesh_quality.txt).

The trained stand-in of scene 102344250 is extracted twice at refine 4: at iso = occ_thre / render_step_size (the reconstruction) and at twice
that iso (a second surface a few millimetres inside the first, which stands in for the ground truth; its sampling at 1 cm is the ground-truth
cloud).  On that pair, medians of `--reps` synchronised calls after two warm-up calls, host clock (the host route: three calls):

  sample_mesh_points(mesh, 0.01)              the reconstruction's own cloud
  nearest(pred, gt, r_max), nearest(gt, pred, r_max)      the two directed searches, the box given (no host copy inside)
  mesh_quality(mesh, gt)                      end to end: sampling, both searches, both reductions, the one copy of the result

and beside them the host route a user has today: both clouds copied to the host, a scipy.spatial.cKDTree built over each and queried with
the other (k = 1, distance_upper_bound = r_max, workers = 16; the builds themselves run on one thread, with scipy's defaults).  Without scipy the device times are recorded alone, and the file says so.

    python tools/mesh_quality_measure.py [--refine 4] [--resolution 0.01] [--threshold 0.05] [--reps 7] [--out profiles/mesh_quality.txt]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import apnrf_amd  # noqa: E402,F401
from apnrf_amd import cloud as CL  # noqa: E402
from apnrf_amd import scenes as SC  # noqa: E402
from apnrf_amd import standin as ST  # noqa: E402
from apnrf_amd import surface as SF  # noqa: E402

DEV = "cuda:0"


def timed(fn, reps, warmup=2):
    """-> (median, min, max) in ms of `reps` synchronised calls after `warmup` calls, and the last result."""
    out = None
    for _ in range(warmup):
        out = fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
    return (float(np.median(ts)), min(ts), max(ts)), out


def fmt(t):
    return f"median {t[0]:9.3f} ms ({t[1]:.3f}-{t[2]:.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--refine", type=int, default=4)
    ap.add_argument("--resolution", type=float, default=0.01)
    ap.add_argument("--threshold", type=float, default=0.05)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mesh_quality_measure needs a GPU: nothing here is a measurement without one")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    scene = SC.make_scene("102344250", n_poses=8)
    field, est, _ = ST.train_standin(scene, DEV)
    iso = 1e-2 / SC.RENDER_KW["render_step_size"]
    mesh = SF.extract_surface(field, est, iso, refine=a.refine)
    truth = SF.extract_surface(field, est, 2.0 * iso, refine=a.refine)
    r_max = 4.0 * a.threshold
    say(f"# mesh quality: each figure is the median (min-max) of {a.reps} synchronised calls after 2 warm-up calls, host clock; one MI355X")
    say(f"meshes   stand-in of scene 102344250, refine {a.refine}: reconstruction (iso {iso:g}) {mesh.n_vertices} vertices, {mesh.n_triangles} triangles; "
        f"ground truth (iso {2 * iso:g}) {truth.n_vertices} vertices, {truth.n_triangles} triangles")
    t_sample, (pred, _) = timed(lambda: CL.sample_mesh_points(mesh, resolution=a.resolution), a.reps)
    gt, gt_face = CL.sample_mesh_points(truth, resolution=a.resolution)
    n, m = int(pred.shape[0]), int(gt.shape[0])
    say(f"sample   sample_mesh_points at {a.resolution:g}: {n} points of the reconstruction, {fmt(t_sample)} (three calls of mnf_cloud_sample_triangles: two "
        f"size the outputs); {n / max(t_sample[0], 1e-9) / 1e3:.1f} M points/s; the ground-truth cloud has {m} points")
    both = torch.cat([pred, gt])
    box = torch.cat([both.amin(dim=0), both.amax(dim=0)]).cpu().numpy()
    t_pg, (d_pg, i_pg) = timed(lambda: CL.nearest(pred, gt, r_max, box=box), a.reps)
    t_gp, (d_gp, i_gp) = timed(lambda: CL.nearest(gt, pred, r_max, box=box), a.reps)
    say(f"nearest  box [{', '.join(f'{x:.3f}' for x in box)}], r_max {r_max:g}")
    say(f"nearest  pred -> gt  ({n} queries, {m} targets): {fmt(t_pg)}; {n / max(t_pg[0], 1e-9) / 1e3:.2f} M queries/s; {int((i_pg < 0).sum())} without a neighbour")
    say(f"nearest  gt -> pred  ({m} queries, {n} targets): {fmt(t_gp)}; {m / max(t_gp[0], 1e-9) / 1e3:.2f} M queries/s; {int((i_gp < 0).sum())} without a neighbour")
    labels = {}
    if mesh.label is not None and truth.label is not None:
        labels = {"gt_labels": truth.label[truth.triangles[:, 0].long()[gt_face.long()]].contiguous()}
    t_all, q = timed(lambda: CL.mesh_quality(mesh, gt, resolution=a.resolution, threshold=a.threshold, **labels), a.reps)
    say(f"quality  mesh_quality end to end (sampling, two searches, two reductions, the copy of the result): {fmt(t_all)}")
    say("quality  " + ", ".join(f"{k} {q[k]:.6g}" for k in ("accuracy", "completion", "completion_ratio", "precision", "recall", "fscore", "chamfer"))
        + f", truncated {q['truncated_pred']} / {q['truncated_gt']}" + (f", label_accuracy {q['label_accuracy']:.4f}, miou {q['miou']:.4f}" if "miou" in q else ""))
    try:
        from scipy.spatial import cKDTree
    except ImportError:
        cKDTree = None
        say("host     scipy is not installed here: the host route (copy + cKDTree.query) was NOT measured; the device times above stand alone")
    if cKDTree is not None:
        def host_route():
            p, g = pred.cpu().numpy(), gt.cpu().numpy()
            t0 = time.perf_counter()
            tp, tg = cKDTree(p), cKDTree(g)
            t1 = time.perf_counter()
            dp, ip = tg.query(p, k=1, distance_upper_bound=r_max, workers=16)
            dg, ig = tp.query(g, k=1, distance_upper_bound=r_max, workers=16)
            host_route.parts = (1e3 * (t1 - t0), 1e3 * (time.perf_counter() - t1))
            return dp, ip, dg, ig
        t_host, (dp, ip, dg, ig) = timed(host_route, 3, warmup=0)
        say(f"host     copy of both clouds + two cKDTree builds + two queries (k = 1, distance_upper_bound = r_max, workers = 16): {fmt(t_host)}; "
            f"the last call: builds {host_route.parts[0]:.1f} ms, queries {host_route.parts[1]:.1f} ms")
        say(f"host     device end to end / host route: {t_all[0] / t_host[0]:.4f} (the device figure includes the sampling and the reductions, the host figure does not)")
        # the clouds repeat every mesh vertex once per triangle around it, so equal distances abound and the tree may name any of them: compare distances
        diff_p = np.abs(np.where(np.isfinite(dp), dp, r_max) - d_pg.cpu().numpy().astype(np.float64)).max()
        diff_g = np.abs(np.where(np.isfinite(dg), dg, r_max) - d_gp.cpu().numpy().astype(np.float64)).max()
        same_p = ((ip == m) == (i_pg.cpu().numpy() < 0)).mean()
        same_g = ((ig == n) == (i_gp.cpu().numpy() < 0)).mean()
        say(f"host     against the k-d tree (float64 distances): largest difference of a distance {diff_p:.3e} pred -> gt, {diff_g:.3e} gt -> pred; "
            f"share of queries found by both or by neither {same_p:.6f}, {same_g:.6f}")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
