"""The quality of the map as geometry, on the device (csrc/cloud.hip): points sampled on the triangles of a mesh as
simulator/build_point_cloud_from_mesh.py samples its ground truth, the nearest neighbour of every point of one cloud in another within a
radius, and accuracy / completion / precision / recall / F-score / Chamfer distance and the class confusion of a reconstructed surface
against a ground-truth cloud.  Only counts and the final numbers visit the host.  The definition is in include/mi355nerf.h ("mesh quality")
and DESIGN.md."""
import ctypes

import numpy as np
import torch

from . import _lib as L


def _temporary(nbytes, dev):
    # a plain temporary, not the per-stream workspace cache (as surface._extract_call): cloud-sized, and an evaluation is a one-off.
    # torch's allocations are 512-byte aligned
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=dev)


def _sample_call(pos, tri, res, max_rows, max_points):
    lib = L.load_library()
    dev = pos.device
    V, T = int(pos.shape[0]), int(tri.shape[0])
    nbytes = int(lib.mnf_cloud_sample_triangles_workspace_bytes(T, max_rows))
    if nbytes <= 0:
        raise L.MnfError(f"{T} triangles with {max_rows} rows are outside [0, 2^31)")
    points = torch.empty(max_points, 3, dtype=torch.float32, device=dev)
    face = torch.empty(max_points, dtype=torch.int32, device=dev)
    info = torch.empty(2, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        ws = _temporary(nbytes, dev)
        L.launch(lib.mnf_cloud_sample_triangles, L.ptr(pos) if V else None, V, L.ptr(tri) if T else None, T, float(res), max_rows, max_points,
                 L.ptr(points) if max_points else None, L.ptr(face) if max_points else None, L.ptr(info), L.ptr(ws), nbytes, device=dev)
    return points, face, info


@torch.no_grad()
def sample_mesh_points(mesh_or_positions, triangles=None, resolution=0.01):
    """Points on the triangles of a mesh, `resolution` apart along two edges of each (the three vertices first): a `SurfaceMesh`, or
    positions [V,3] float32 and triangles [T,3] int32 on the device -> (points float32 [P,3], face int32 [P], the triangle of each point) on
    the device, in ascending (triangle, vertices, row, column).  Two small host copies size the workspace and the outputs (rows, then points)."""
    if triangles is None:
        mesh_or_positions, triangles = mesh_or_positions.positions, mesh_or_positions.triangles
    L.require_gpu(mesh_or_positions, triangles)
    pos = L.contig(mesh_or_positions.reshape(-1, 3), torch.float32)
    tri = L.contig(triangles.reshape(-1, 3), torch.int32)
    if not resolution > 0:
        raise ValueError(f"resolution must be positive (got {resolution})")
    # the rows first (a call with no row capacity costs one lane per triangle and reports them), then the points of exactly those rows, then
    # the fill: the workspace and the per-row passes are as large as the mesh's rows, not as a guess
    max_rows = 0
    host = _sample_call(pos, tri, resolution, 0, 0)[2].cpu().numpy()
    if host[0] < 0:
        max_rows = int(host[1])
        if max_rows > 0x7fffffff:
            raise L.MnfError(f"the mesh has {max_rows} sampling rows at resolution {resolution}: more than 2^31 - 1")
        host = _sample_call(pos, tri, resolution, max_rows, 0)[2].cpu().numpy()
    n = int(host[0])
    if n > 0x7fffffff:
        raise L.MnfError(f"the mesh has at least {n} points at resolution {resolution}: more than 2^31 - 1")
    points, face, info = _sample_call(pos, tri, resolution, max_rows, n)
    return points, face


def _box6(box, *clouds):
    if box is None:                                                  # the extent of the finite points: two reductions per cloud, one 24-byte copy
        ends = []
        for c in clouds:
            if int(c.shape[0]) == 0:
                continue
            ok = torch.isfinite(c).all(dim=1, keepdim=True)
            ends.append(torch.cat([torch.where(ok, c, float("inf")).amin(dim=0), -torch.where(ok, c, float("-inf")).amax(dim=0)]))
        box = np.zeros(6, np.float32)
        if ends:
            e = torch.stack(ends).amin(dim=0).cpu().numpy()
            if np.isfinite(e).all():                                 # else no finite point at all: any box will do
                box = np.concatenate([e[:3], -e[3:]])
    a = np.asarray(box.detach().cpu().numpy() if isinstance(box, torch.Tensor) else box, np.float32).reshape(6)
    return (ctypes.c_float * 6)(*[float(x) for x in a])


def _nearest_call(q, t, r_max, box6):
    lib = L.load_library()
    dev = q.device
    n, m = int(q.shape[0]), int(t.shape[0])
    nbytes = int(lib.mnf_cloud_nearest_workspace_bytes(n, m, box6, float(r_max)))
    if nbytes <= 0:
        raise L.MnfError(f"nearest: {n} queries, {m} targets, r_max = {r_max}, box = {list(box6)}: counts are < 2^31, r_max > 0, the box finite with max >= min")
    index = torch.empty(n, dtype=torch.int32, device=dev)
    dist = torch.empty(n, dtype=torch.float32, device=dev)
    if n:
        with torch.cuda.device(dev):
            ws = _temporary(nbytes, dev)
            L.launch(lib.mnf_cloud_nearest, L.ptr(q), n, L.ptr(t) if m else None, m, float(r_max), box6, L.ptr(index), L.ptr(dist), L.ptr(ws), nbytes, device=dev)
    return dist, index


@torch.no_grad()
def nearest(query, target, r_max, box=None):
    """For every point of `query` [n,3] the nearest point of `target` [m,3] (float32, on the device) within `r_max` -> (dist float32 [n],
    index int32 [n]); index -1 and dist r_max where there is none.  Exactly the brute-force answer in float32, the lowest index on a tie.
    `box` (min, max: six numbers) places the cell list and should hug the targets; None takes the targets' own extent (one small host copy)."""
    L.require_gpu(query, target)
    q = L.contig(query.reshape(-1, 3), torch.float32)
    t = L.contig(target.reshape(-1, 3), torch.float32)
    return _nearest_call(q, t, r_max, _box6(box, t))


def _stats_call(dist, index, query, thr, r_max, m, query_label=None, target_label=None, C=0):
    dev = dist.device
    n = int(dist.shape[0])
    out = torch.empty(5 + C * C, dtype=torch.int64, device=dev)     # counts [3], sums [2] (float64 bits), confusion [C,C]: one buffer, one copy
    counts, sums, conf = out[:3], out[3:5], out[5:] if C else None
    L.launch(L.load_library().mnf_cloud_distance_stats, L.ptr(dist) if n else None, L.ptr(index) if n else None, L.ptr(query) if n else None, n, float(thr),
             float(r_max), L.ptr(query_label) if C and n else None, L.ptr(target_label) if C and m else None, m, C, L.ptr(counts), L.ptr(sums), L.ptr(conf),
             device=dev)
    return out


def _labels(t, n, dev):
    if t is None:
        return None
    t = L.contig(t.reshape(-1).to(dev), torch.int32)
    if int(t.shape[0]) != n:
        raise ValueError(f"{int(t.shape[0])} labels for {n} points")
    return t


@torch.no_grad()
def mesh_quality(pred, gt_points, gt_labels=None, pred_labels=None, resolution=0.01, threshold=0.05, r_max=None, num_classes=None):
    """The reconstructed surface `pred` against the ground-truth cloud `gt_points` [m,3] (float32, on the device).

    `pred` is a `SurfaceMesh` or a point tensor [n,3].  A mesh is sampled first (`sample_mesh_points` at `resolution`) and each sampled
    point takes the label of its triangle's first vertex (`pred_labels` per VERTEX, default the mesh's own `label`); for a point tensor
    `pred_labels` is per point.  Two directed searches, pred -> gt and gt -> pred, within `r_max` (default 4 x threshold: an API default,
    not a measurement); a point with no neighbour within r_max counts with the distance r_max, and `truncated_*` say how many did.
    -> dict of host numbers:
      accuracy          mean distance pred -> gt            completion        mean distance gt -> pred
      precision         share of pred within `threshold`    recall = completion_ratio   share of gt within `threshold`
      fscore            2 P R / (P + R)                      chamfer           (accuracy + completion) / 2
      n_pred, n_gt      the finite points of either cloud   truncated_pred, truncated_gt   those without a neighbour within r_max
    and with labels on both sides (`num_classes` = C, default 1 + the largest label): confusion int64 [C,C] over the gt points within
    `threshold` (row: the gt label, column: the label of the nearest predicted point), label_accuracy = trace / sum, miou = the mean
    over the classes that occur of intersection / union.  Everything is reduced on the device and one small copy at the end brings the result.  Before it the
    call synchronises for a few words only: the two sizing copies of a mesh's sampling, the 24-byte box of the two clouds, and, when
    `num_classes` is not given, the two largest labels."""
    L.require_gpu(gt_points)
    gt = L.contig(gt_points.reshape(-1, 3), torch.float32)
    dev = gt.device
    if r_max is None:
        r_max = 4.0 * float(threshold)
    if not 0 <= threshold <= r_max:
        raise ValueError(f"threshold must lie in [0, r_max] (got {threshold}, r_max {r_max})")
    if isinstance(pred, torch.Tensor):
        L.require_gpu(pred)
        points = L.contig(pred.reshape(-1, 3), torch.float32)
        plabel = _labels(pred_labels, int(points.shape[0]), dev)
    else:
        points, face = sample_mesh_points(pred, resolution=resolution)
        vlabel = pred_labels if pred_labels is not None else getattr(pred, "label", None)
        plabel = None
        if vlabel is not None:
            vlabel = _labels(vlabel, int(pred.positions.shape[0]), dev)
            plabel = vlabel[pred.triangles[:, 0].long()[face.long()]].contiguous()
    glabel = _labels(gt_labels, int(gt.shape[0]), dev)
    with_labels = plabel is not None and glabel is not None
    C = 0
    if with_labels:
        C = int(num_classes) if num_classes is not None else int(max(int(plabel.max()) if plabel.numel() else -1, int(glabel.max()) if glabel.numel() else -1)) + 1
        C = max(C, 1)
    n, m = int(points.shape[0]), int(gt.shape[0])
    box6 = _box6(None, points, gt)
    d_pg, i_pg = _nearest_call(points, gt, r_max, box6)
    d_gp, i_gp = _nearest_call(gt, points, r_max, box6)
    s_pg = _stats_call(d_pg, i_pg, points, threshold, r_max, m)
    s_gp = _stats_call(d_gp, i_gp, gt, threshold, r_max, n, glabel, plabel, C)
    host = torch.cat([s_pg, s_gp]).cpu().numpy()
    c_pg, sum_pg = host[:3], host[3:5].view(np.float64)
    c_gp, sum_gp = host[5:8], host[8:10].view(np.float64)

    def ratio(a, b):
        return float(a) / float(b) if b else float("nan")

    out = {"accuracy": ratio(sum_pg[0], c_pg[0]), "completion": ratio(sum_gp[0], c_gp[0]), "precision": ratio(c_pg[2], c_pg[0]),
           "recall": ratio(c_gp[2], c_gp[0]), "n_pred": int(c_pg[0]), "n_gt": int(c_gp[0]), "truncated_pred": int(c_pg[0] - c_pg[1]),
           "truncated_gt": int(c_gp[0] - c_gp[1]), "threshold": float(threshold), "r_max": float(r_max)}
    out["completion_ratio"] = out["recall"]
    p, r = out["precision"], out["recall"]
    out["fscore"] = 2.0 * p * r / (p + r) if p + r > 0 else (0.0 if p + r == 0 else float("nan"))
    out["chamfer"] = 0.5 * (out["accuracy"] + out["completion"])
    if with_labels:
        conf = host[10:].reshape(C, C).copy()
        inter = np.diag(conf).astype(np.float64)
        union = conf.sum(axis=0) + conf.sum(axis=1) - np.diag(conf)
        out["confusion"] = conf
        out["label_accuracy"] = ratio(inter.sum(), conf.sum())
        out["miou"] = float((inter[union > 0] / union[union > 0]).mean()) if (union > 0).any() else float("nan")
    return out


_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2", "uint16": "u2", "int": "i4", "int32": "i4",
              "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4", "double": "f8", "float64": "f8"}


def load_point_cloud_ply(path):
    """The numpy reader of a point cloud PLY such as simulator/build_point_cloud_from_mesh.py writes: ascii or binary_little_endian,
    `x y z` as float or double, optional `uchar red green blue`; other vertex properties are skipped and other elements ignored (the
    vertex element must come first).  -> dict(points float32 [n,3], colour uint8 [n,3] or None)."""
    with open(path, "rb") as fh:
        data = fh.read()
    mark = data.find(b"end_header")
    if not data.startswith(b"ply") or mark < 0:
        raise ValueError(f"{path} is not a PLY file")
    end = data.index(b"\n", mark) + 1
    lines = [ln.strip() for ln in data[:end].decode("ascii").splitlines()]
    fmt = next((ln.split()[1] for ln in lines if ln.startswith("format ")), None)
    if fmt not in ("ascii", "binary_little_endian"):
        raise ValueError(f"{path}: format {fmt!r} is neither ascii nor binary_little_endian")
    element, n, props = None, 0, []
    first = True
    for ln in lines:
        w = ln.split()
        if not w:
            continue
        if w[0] == "element":
            if element == "vertex":
                break
            if not first or w[1] != "vertex":
                raise ValueError(f"{path}: the first element is {w[1]!r}, not vertex")
            element, n, first = w[1], int(w[2]), False
        elif w[0] == "property" and element == "vertex":
            if w[1] == "list":
                raise ValueError(f"{path}: a list property in the vertex element")
            if w[1] not in _PLY_TYPES:
                raise ValueError(f"{path}: property type {w[1]!r}")
            props.append((w[2], _PLY_TYPES[w[1]]))
    names = [p[0] for p in props]
    if element != "vertex" or not all(k in names for k in "xyz"):
        raise ValueError(f"{path}: no vertex element with x, y, z")
    for k in "xyz":
        if dict(props)[k] not in ("f4", "f8"):
            raise ValueError(f"{path}: {k} is neither float nor double")
    if fmt == "ascii":
        rows = data[end:].split(b"\n")[:n]
        table = np.array([r.split() for r in rows], dtype=np.float64).reshape(n, len(props)) if n else np.zeros((0, len(props)))
        col = {name: table[:, i] for i, name in enumerate(names)}
    else:
        dt = np.dtype([(name, "<" + t) for name, t in props])
        if len(data) < end + n * dt.itemsize:
            raise ValueError(f"{path}: {len(data) - end} bytes for {n} vertices of {dt.itemsize} bytes")
        rec = np.frombuffer(data, dt, n, end)
        col = {name: rec[name] for name in names}
    points = np.stack([np.asarray(col[k], np.float32) for k in "xyz"], axis=1) if n else np.zeros((0, 3), np.float32)
    colour = None
    if all(k in names for k in ("red", "green", "blue")) and all(dict(props)[k] == "u1" for k in ("red", "green", "blue")):
        colour = np.stack([np.asarray(col[k]).astype(np.uint8) for k in ("red", "green", "blue")], axis=1) if n else np.zeros((0, 3), np.uint8)
    return {"points": np.ascontiguousarray(points), "colour": colour}
