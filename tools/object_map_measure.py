"""Measurement of the semantic object map (profiles/object_map.txt): 40 views of 640 x 640 pixels with C = 29 logits
inserted into the box of scene 102344280 at 0.1 m voxels, then the clusters of that map and their match to 200 objects.

The planes are synthetic and seeded (no field is trained): the cameras sweep the yaw within 4 m of the scene's origin, a pixel's depth is the length
of its ray to the walls of the box shrunk by half a metre, its class a hash of the 1.5 m block of wall it hits, its logits that class
at +4 over unit noise.  That gives what a finished run gives the map: surfaces seen many times over, patches of classes on them.

  1. `mnf_object_map_insert` (device events around the call, legs interleaved in one loop): into a cleared map (every new voxel takes
     its atomic OR) and into the map that already holds the same views (a plain load per pixel), logits and u8 labels, beside the bytes
     each must read over the 8 TB/s HBM figure.
  2. `mnf_object_map_clusters` and `mnf_object_map_match` (device events), and the wall time of `SemanticObjectMap.detect` with its
     count read-back and host copy.
  3. The numpy restatement tests/objmap_ref.py on the same arrays on the host of the GPU box (once: it is seconds of Python loops), and whether
     both give the same bits, rows and matches.

    python tools/object_map_measure.py [--views 40] [--reps 9] [--out FILE]
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
import apnrf_amd  # noqa: E402,F401
import objmap_ref as OR  # noqa: E402
from apnrf_amd import render as RD  # noqa: E402
from apnrf_amd import synthetic as S  # noqa: E402
from apnrf_amd.objects import SemanticObjectMap  # noqa: E402

DEV = "cuda:0"
SCENE = "102344280"
W = H = 640
C = 29
HBM = 8.0e12


def synthetic_planes(n_views, aabb):
    """-> rays_o, rays_d [N,3], depth [N], acc [N], sem [N,C], labels [N] u8 on the device"""
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
    p = o + t[:, None] * d
    blk = torch.floor(p / 1.5).to(torch.int64)
    cls = ((blk[:, 0] * 73856093) ^ (blk[:, 1] * 19349663) ^ (blk[:, 2] * 83492791)).remainder(C)
    g = torch.Generator(device=DEV).manual_seed(0)
    sem = torch.randn(o.shape[0], C, device=DEV, generator=g)
    sem[torch.arange(o.shape[0], device=DEV), cls] += 4.0
    acc = torch.rand(o.shape[0], device=DEV, generator=g) * 0.5 + 0.5
    return o.contiguous(), d.contiguous(), t.contiguous(), acc, sem, sem.argmax(-1).to(torch.uint8)


def event_ms(legs, reps, warmup=2):
    """legs: name -> (prepare or None, fn).  Every repetition runs every leg once, in order; -> name -> (median, min, max) ms of device time."""
    times = {k: [] for k in legs}
    for r in range(warmup + reps):
        for name, (prep, fn) in legs.items():
            if prep:
                prep()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if r >= warmup:
                times[name].append(a.elapsed_time(b))
    return {k: (float(np.median(v)), float(np.min(v)), float(np.max(v))) for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=40)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-host", action="store_true", help="skip the numpy restatement")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("object_map_measure needs a GPU: nothing here is a measurement without one")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    aabb = S.SCENES[SCENE]["aabb"]
    o, d, depth, acc, sem, lab = synthetic_planes(a.views, aabb)
    N = int(depth.shape[0])
    m = SemanticObjectMap(aabb, voxel_size=0.1, num_classes=C, device=DEV)
    kw = dict(min_depth=0.05, max_depth=50.0, min_acc=0.5)
    say(f"# semantic object map: {a.views} views of {W}x{H} = {N} pixels, C = {C}, box of scene {SCENE} at 0.1 m: {m.resolution} voxels x {C} planes = "
        f"{m.bits.numel() * 4 / 1e6:.1f} MB of bits; medians of {a.reps} repetitions (min-max), legs interleaved, device events")
    # ---- 1. insert
    legs = {"logits, cleared map": (m.clear, lambda: m.insert(o, d, depth, sem=sem, acc=acc, **kw)),
            "logits, map already set": (None, lambda: m.insert(o, d, depth, sem=sem, acc=acc, **kw)),
            "u8 labels, cleared map": (m.clear, lambda: m.insert(o, d, depth, labels=lab, acc=acc, **kw)),
            "u8 labels, map already set": (None, lambda: m.insert(o, d, depth, labels=lab, acc=acc, **kw))}
    res = event_ms(legs, a.reps)
    for name, (med, lo, hi) in res.items():
        per = 12 + 12 + 4 + 4 + (4 * C if name.startswith("logits") else 1)
        floor_ms = 1e3 * per * N / HBM
        say(f"mnf_object_map_insert  {name:28s} {med:8.3f} ms ({lo:.3f}-{hi:.3f}) | {per} B read per pixel = {per * N / 1e9:.2f} GB -> {floor_ms:.3f} ms at 8 TB/s "
            f"({floor_ms / med:.2f} of it); {per * N / med / 1e9:.2f} TB/s")
    m.clear()
    m.insert(o, d, depth, sem=sem, acc=acc, **kw)
    counts = m.voxel_counts().cpu().numpy()
    M = int(counts.sum())
    say(f"map: {M} set voxels in {int((counts > 0).sum())} classes (largest class {int(counts.max())})")
    # ---- 2. clusters and match
    rng = np.random.default_rng(0)
    box = np.asarray(aabb, np.float64)
    G = 200
    gt_locs = rng.uniform(box[:3], box[3:], (G, 3))
    gt_cls = rng.integers(1, C, G).astype(np.int32)
    lib = apnrf_amd.load_library()
    from apnrf_amd import _lib as L
    dev_out = {}
    d_locs, d_cls = torch.from_numpy(gt_locs).to(DEV), torch.from_numpy(gt_cls).to(DEV)
    detected = torch.empty(C, dtype=torch.int32, device=DEV)
    match = torch.empty(M, dtype=torch.int32, device=DEV)
    gt_match = torch.empty(G, dtype=torch.int32, device=DEV)

    def run_clusters():
        dev_out.update(m._clusters_device(4, 1, True, max_voxels=M, max_clusters=M))

    def run_match():
        L.launch(lib.mnf_object_map_match, L.ptr(dev_out["clusters"]), L.ptr(dev_out["info"]), M, C, L.ptr(d_locs), L.ptr(d_cls), G, 1.0, L.ptr(detected),
                 L.ptr(match), L.ptr(gt_match))

    res = event_ms({"clusters": (None, run_clusters), "match": (None, run_match), "count": (None, m.voxel_counts)}, a.reps)
    grid_bytes = m.bits.numel() * 4
    need = 3 * grid_bytes + 16 * m.bits.numel() + 60 * M
    say(f"mnf_object_map_clusters  link_r2=4, labelled cloud: {res['clusters'][0]:8.3f} ms ({res['clusters'][1]:.3f}-{res['clusters'][2]:.3f}) | reads the "
        f"{grid_bytes / 1e6:.1f} MB grid 3 times + 16 B of scan state per word + ~60 B per set voxel = {need / 1e6:.1f} MB -> {1e3 * need / HBM:.4f} ms at 8 TB/s")
    say(f"mnf_object_map_count     {res['count'][0]:8.3f} ms ({res['count'][1]:.3f}-{res['count'][2]:.3f}) | {grid_bytes / 1e6:.1f} MB -> {1e3 * grid_bytes / HBM:.4f} ms at 8 TB/s")
    info = dev_out["info"].cpu().numpy()
    say(f"mnf_object_map_match     {G} objects, {int(info[1])} clusters: {res['match'][0]:8.3f} ms ({res['match'][1]:.3f}-{res['match'][2]:.3f}) | one wave per class, "
        f"sequential over a class's clusters (latency-bound: {(int(info[1]) * 40 + G * 28) / 1e3:.1f} KB of data)")
    ts = []
    for _ in range(a.reps + 1):
        t0 = time.perf_counter()
        got = m.detect(gt_locs, gt_cls, det_dist_thresh=1.0)
        ts.append(1e3 * (time.perf_counter() - t0))
    say(f"wall  SemanticObjectMap.detect (count read-back, clusters, match, host copy): {np.median(ts[1:]):8.3f} ms ({min(ts[1:]):.3f}-{max(ts[1:]):.3f}); "
        f"{got['total']} of {G} objects detected, {len(got['class'])} clusters")
    # ---- 3. the numpy restatement on this host
    if not a.no_host:
        ho, hd, hdep, hacc, hsem = (t.cpu().numpy() for t in (o, d, depth, acc, sem))
        t0 = time.perf_counter()
        want = OR.insert(np.zeros((C, m.words_per_plane), np.uint32), ho, hd, hdep, m.grid_min, m.voxel_size, m.resolution, sem=hsem, acc=hacc, **kw)
        t_ins = time.perf_counter() - t0
        same_bits = np.array_equal(m.bits.cpu().numpy().view(np.uint32), want)
        t0 = time.perf_counter()
        ref = OR.clusters(want, m.resolution, m.grid_min, m.voxel_size, link_r2=4)
        t_clu = time.perf_counter() - t0
        t0 = time.perf_counter()
        det, mt, gm = OR.match(ref["rows"], C, gt_locs, gt_cls, 1.0)
        t_mat = time.perf_counter() - t0
        same_rows = np.array_equal(ref["rows"][:, 2:], got["centroid"]) and np.array_equal(ref["rows"][:, 1].astype(np.int64), got["count"])
        same_match = np.array_equal(det, got["detected"]) and np.array_equal(mt, got["match"]) and np.array_equal(gm, got["gt_match"])
        say(f"host  tests/objmap_ref.py on the same arrays, once ({os.cpu_count()} CPUs, numpy {np.__version__}): insert {1e3 * t_ins:.0f} ms, clusters "
            f"{1e3 * t_clu:.0f} ms, match {1e3 * t_mat:.0f} ms | same bits {same_bits}, same rows {same_rows}, same match {same_match}")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
