"""Measurement of the exploration map (DESIGN.md "Exploration map", profiles/exploration_map.txt): 40 views of 640 x 640 pixels, one planning
step's addition, ray-cast into the box of scene 102344250 at 0.1 m voxels with max_range 10, then the read-outs of that map.

The planes are synthetic and seeded as in tools/object_map_measure.py (no field is trained): the cameras sweep the yaw within 4 m of the scene's
origin, a pixel's depth is the length of its ray to the walls of the box shrunk by half a metre; rays longer than max_range only carve.

  1. `mnf_explore_map_insert` (device events around the call, legs interleaved in one loop) into a cleared map and into the map that the same
     views have already carved, each beside `mnf_object_map_insert` with u8 labels on the same pixels (the end-point-only floor); from the
     kernel's own counters the mean steps per ray and the atomic ORs issued per bit newly set.
  2. The read-outs, each timed: count, top-down, frontiers, frontier clusters, and the wall time of `ExplorationMap.frontier_goals`.
  3. The numpy restatement tests/explore_ref.py on the host for the arrays of the first --host-views views (the whole walk in numpy is minutes
     for all 40), and whether a device map of those views has the same bits.

    python tools/exploration_map_measure.py [--views 40] [--reps 9] [--host-views 2] [--out FILE]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tools"))
import apnrf_amd  # noqa: E402,F401
import explore_ref as ER  # noqa: E402
from apnrf_amd import _lib as L  # noqa: E402
from apnrf_amd import render as RD  # noqa: E402
from apnrf_amd import synthetic as S  # noqa: E402
from apnrf_amd.explore import ExplorationMap  # noqa: E402
from apnrf_amd.objects import SemanticObjectMap  # noqa: E402
from object_map_measure import event_ms  # noqa: E402

DEV = "cuda:0"
SCENE = "102344250"
W = H = 640
MAX_RANGE = 10.0
HBM = 8.0e12


def synthetic_planes(n_views, aabb):
    """-> rays_o, rays_d [N,3], depth [N], acc [N], labels [N] u8 on the device"""
    poses = S.camera_poses(S.SCENES[SCENE]["origin"], n_views, radius=4.0)
    c2w = np.stack([RD.pose_to_c2w(np.asarray(p, np.float64)) for p in poses]).astype(np.float32)
    focal = 0.5 * W / np.tan(np.pi / 4)
    K = np.array([[focal, 0.0, W / 2], [0.0, focal, H / 2], [0.0, 0.0, 1.0]])
    rays = RD.generate_image_rays(torch.from_numpy(c2w), W, H, K, DEV)
    o, d = rays.origins.reshape(-1, 3), rays.viewdirs.reshape(-1, 3)
    box = torch.tensor(aabb, device=DEV)
    lo, hi = box[:3] + 0.5, box[3:] - 0.5
    far = torch.where(d > 0, hi, lo)
    t = ((far - o) / torch.where(d == 0, torch.full_like(d, 1e-9), d)).amin(dim=1)
    g = torch.Generator(device=DEV).manual_seed(0)
    acc = torch.rand(o.shape[0], device=DEV, generator=g) * 0.5 + 0.5
    lab = torch.ones(o.shape[0], dtype=torch.uint8, device=DEV)
    return o.contiguous(), d.contiguous(), t.contiguous(), acc, lab, np.asarray(poses[0], np.float64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=40)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--host-views", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("exploration_map_measure needs a GPU: nothing here is a measurement without one")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    aabb = S.SCENES[SCENE]["aabb"]
    o, d, depth, acc, lab, pose0 = synthetic_planes(a.views, aabb)
    N = int(depth.shape[0])
    m = ExplorationMap(aabb, voxel_size=0.1, max_range=MAX_RANGE, device=DEV)
    om = SemanticObjectMap(aabb, voxel_size=0.1, num_classes=2, device=DEV)
    kw = dict(min_depth=0.05, min_acc=0.5)
    say(f"# exploration map: {a.views} views of {W}x{H} = {N} pixels, box of scene {SCENE} at 0.1 m: {m.resolution} voxels x 2 planes = "
        f"{m.bits.numel() * 4 / 1e6:.2f} MB of bits, max_range {MAX_RANGE}; medians of {a.reps} repetitions (min-max), legs interleaved, device events")
    beyond = float((depth > MAX_RANGE).float().mean())
    say(f"depths: median {float(depth.median()):.2f} m, {100 * beyond:.1f} % beyond max_range (those only carve)")
    # ---- 1. insert
    legs = {"explore, cleared map": (m.clear, lambda: m.insert(o, d, depth, acc=acc, **kw)),
            "explore, map already carved": (None, lambda: m.insert(o, d, depth, acc=acc, **kw)),
            "object map u8, cleared map": (om.clear, lambda: om.insert(o, d, depth, labels=lab, acc=acc, max_depth=MAX_RANGE, **kw)),
            "object map u8, map already set": (None, lambda: om.insert(o, d, depth, labels=lab, acc=acc, max_depth=MAX_RANGE, **kw))}
    res = event_ms(legs, a.reps)
    # the kernel's counters, outside the timed loop: steps walked and ORs issued, into a cleared and into a carved map
    stats = torch.zeros(2, dtype=torch.int64, device=DEV)
    m.clear()
    m.insert(o, d, depth, acc=acc, stats=stats, **kw)
    steps0, ors0 = stats.tolist()
    c = m.counts()
    new_bits = c["free"] + c["occupied"]
    set_bits = int(np.unpackbits(m.bits.cpu().numpy().view(np.uint8)).sum())                      # both planes: an occupied voxel that is also passed through has two
    stats.zero_()
    m.insert(o, d, depth, acc=acc, stats=stats, **kw)
    steps1, ors1 = stats.tolist()
    per = 12 + 12 + 4 + 4
    for name, (med, lo, hi) in res.items():
        say(f"insert  {name:32s} {med:9.3f} ms ({lo:.3f}-{hi:.3f}) | {N / med / 1e6:.2f} G pixels/s; {per} B read per pixel -> "
            f"{1e3 * per * N / HBM:.3f} ms at 8 TB/s")
    e0, e1 = res["explore, cleared map"][0], res["explore, map already carved"][0]
    f0, f1 = res["object map u8, cleared map"][0], res["object map u8, map already set"][0]
    say(f"explore / end-point-only floor: cleared {e0 / f0:.1f}x, carved {e1 / f1:.1f}x")
    say(f"walk: {steps0 / N:.1f} steps per pixel ({steps0 / 1e9:.2f} G steps: {steps0 / e0 / 1e6:.1f} G steps/s cleared, {steps1 / e1 / 1e6:.1f} G steps/s carved)")
    say(f"ORs, cleared map: {ors0} issued for {set_bits} bits newly set ({new_bits} voxels seen) = {ors0 / max(set_bits, 1):.2f} per bit, "
        f"{ors0 / N:.2f} per pixel; carved map: {ors1} issued for 0 new bits ({ors1 / N:.4f} per pixel)")
    say(f"map: {c['free']} free, {c['occupied']} occupied, {c['unknown']} unknown voxels; explored volume {c['explored_volume']:.1f} m^3")
    # ---- 2. read-outs
    X, _, Z = m.resolution
    lib = apnrf_amd.load_library()
    hold = {}

    def run_topdown():
        hold["td"] = m.top_down()

    def run_frontiers():
        hold["fr"] = m._frontiers_device(hold["td"], None)

    mf = X * Z
    labels = torch.empty(mf, dtype=torch.int32, device=DEV)
    goals = torch.empty(mf, 2, dtype=torch.int32, device=DEV)
    sizes = torch.empty(mf, dtype=torch.int32, device=DEV)
    info = torch.empty(2, dtype=torch.int64, device=DEV)
    nbytes = int(lib.mnf_explore_map_frontier_clusters_workspace_bytes(X, Z, mf, mf))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    cur = m.cell_of((pose0[0], pose0[2]))

    def run_clusters():
        f = hold["fr"]
        L.launch(lib.mnf_explore_map_frontier_clusters, L.ptr(f["cells"]), L.ptr(f["mult"]), L.ptr(f["info"]), mf, X, Z, 1, 3, 1, float(cur[0]), float(cur[1]),
                 mf, L.ptr(labels), L.ptr(goals), L.ptr(sizes), L.ptr(info), L.ptr(ws), nbytes)

    res = event_ms({"count": (None, m.counts_device), "topdown": (None, run_topdown), "frontiers": (None, run_frontiers), "clusters": (None, run_clusters)},
                   a.reps)
    grid_bytes = m.bits.numel() * 4
    say(f"mnf_explore_map_count              {res['count'][0]:8.3f} ms ({res['count'][1]:.3f}-{res['count'][2]:.3f}) | {grid_bytes / 1e6:.2f} MB -> "
        f"{1e3 * grid_bytes / HBM:.4f} ms at 8 TB/s (a memset and a launch)")
    say(f"mnf_explore_map_topdown            {res['topdown'][0]:8.3f} ms ({res['topdown'][1]:.3f}-{res['topdown'][2]:.3f}) | {X} x {Z} cells, all layers")
    F, K = int(hold["fr"]["info"][0]), int(info[0])
    say(f"mnf_explore_map_frontiers          {res['frontiers'][0]:8.3f} ms ({res['frontiers'][1]:.3f}-{res['frontiers'][2]:.3f}) | one workgroup, "
        f"{-(-X * Z // 1024)} batches of 1024 cells in order; {F} frontier cells")
    say(f"mnf_explore_map_frontier_clusters  {res['clusters'][0]:8.3f} ms ({res['clusters'][1]:.3f}-{res['clusters'][2]:.3f}) | capacity {mf} cells, nine launches "
        f"and a scan; {K} clusters")
    ts = []
    for _ in range(a.reps + 1):
        t0 = time.perf_counter()
        got = m.frontier_goals((pose0[0], pose0[2]))
        ts.append(1e3 * (time.perf_counter() - t0))
    say(f"wall  ExplorationMap.frontier_goals (top-down, frontiers, clusters, host copy): {np.median(ts[1:]):8.3f} ms ({min(ts[1:]):.3f}-{max(ts[1:]):.3f}); "
        f"{len(got['goal_cells'])} goals")
    # ---- 3. the numpy restatement on this host, the first views only
    if a.host_views > 0:
        n = min(a.host_views, a.views) * W * H
        sub = ExplorationMap(aabb, voxel_size=0.1, max_range=MAX_RANGE, device=DEV)
        sub.insert(o[:n], d[:n], depth[:n], acc=acc[:n], **kw)
        ho, hd, hdep, hacc = (t[:n].cpu().numpy() for t in (o, d, depth, acc))
        t0 = time.perf_counter()
        want = ER.insert(ER.new_bits(sub.resolution), ho, hd, hdep, sub.grid_min, sub.voxel_size, sub.resolution, MAX_RANGE, acc=hacc, **kw)
        t_ins = time.perf_counter() - t0
        same_bits = np.array_equal(sub.bits.cpu().numpy().view(np.uint32), want)
        t0 = time.perf_counter()
        td = ER.top_down(want, sub.resolution)
        cells, mult, _ = ER.frontiers(td)
        fc = ER.frontier_clusters(cells, mult, sub.cell_of((pose0[0], pose0[2])))
        t_read = time.perf_counter() - t0
        g = sub.frontier_goals((pose0[0], pose0[2]))
        same_read = (np.array_equal(g["cells"], cells) and np.array_equal(g["mult"], mult) and np.array_equal(g["labels"], fc["labels"])
                     and np.array_equal(g["goal_cells"], fc["goals"]) and np.array_equal(g["sizes"], fc["sizes"]))
        say(f"host  tests/explore_ref.py on the arrays of the first {n // (W * H)} views ({n} pixels), once ({os.cpu_count()} CPUs, numpy {np.__version__}): insert "
            f"{1e3 * t_ins:.0f} ms, top-down + frontiers + clusters {1e3 * t_read:.0f} ms | same bits {same_bits}, same frontiers, labels and goals {same_read}")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
