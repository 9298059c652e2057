"""A plain numpy restatement of include/mi355nerf.h ("mesh quality"): points sampled on triangles, the nearest neighbour within a radius by
brute force over all pairs, and the reduction of the distances.  tests/test_cloud_cpu.py holds it to known answers; tests/test_gpu_cloud.py
holds the device (csrc/cloud.hip) to it."""
import math

import numpy as np

CAP = 1 << 31


def _count(x):
    """ceil(x) as a count: 0 for x <= 0 and NaN (numpy's arange of such a length is empty), saturating at 2^31."""
    if not x > 0.0:
        return 0
    return int(min(math.ceil(x), CAP)) if math.isfinite(x) else CAP


def _norm(e):
    return np.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])


def triangle_ratios(positions, triangles, res):
    """Every d1 / res and b / res a sampling evaluates, as float64: a test asserts that none lies next to an integer."""
    out = []
    for tri in np.asarray(triangles):
        if (tri < 0).any() or (tri >= len(positions)).any():
            continue
        v = np.asarray(positions, np.float32)[tri]
        if not np.isfinite(v).all():
            continue
        p = v.astype(np.float64)
        d1, d2 = _norm(p[1] - p[0]), _norm(p[2] - p[0])
        if d1 == 0.0 or d2 == 0.0:
            continue
        out.append(d1 / res)
        for k in range(_count(d1 / res)):
            i = np.float64(k) * res
            out.append(((d1 - i) * d2) / d1 / res)
    return np.array(out, np.float64)


def triangle_rows(positions, triangles, res):
    """The rows of the header's layout: 0 for a triangle with a bad index, 1 for one that gives its vertices only, else 1 + count(d1 / res)."""
    positions = np.asarray(positions, np.float32)
    rows = 0
    for tri in np.asarray(triangles):
        if (tri < 0).any() or (tri >= len(positions)).any():
            continue
        rows += 1
        v = positions[tri]
        if not np.isfinite(v).all():
            continue
        p = v.astype(np.float64)
        d1, d2 = _norm(p[1] - p[0]), _norm(p[2] - p[0])
        if d1 != 0.0 and d2 != 0.0:
            rows += _count(d1 / np.float64(res))
    return rows


def sample_triangles(positions, triangles, res):
    """-> points float32 [P,3], face int32 [P] in ascending (triangle, vertices, k, l)."""
    positions = np.asarray(positions, np.float32)
    res = np.float64(res)
    pts, face = [], []
    with np.errstate(all="ignore"):
        for t, tri in enumerate(np.asarray(triangles)):
            if (tri < 0).any() or (tri >= len(positions)).any():
                continue
            v = positions[tri]
            pts.append(v.copy())
            face.append(np.full(3, t, np.int32))
            if not np.isfinite(v).all():
                continue
            p = v.astype(np.float64)
            e1, e2 = p[1] - p[0], p[2] - p[0]
            d1, d2 = _norm(e1), _norm(e2)
            if d1 == 0.0 or d2 == 0.0:
                continue
            n1, n2 = e1 / d1, e2 / d2
            for k in range(_count(d1 / res)):
                i = np.float64(k) * res
                b = ((d1 - i) * d2) / d1
                n = _count(b / res)
                if n == 0:
                    continue
                j = np.arange(n, dtype=np.float64) * res
                row = (p[0][None, :] + i * n1[None, :]) + j[:, None] * n2[None, :]
                pts.append(row.astype(np.float32))
                face.append(np.full(n, t, np.int32))
    if not pts:
        return np.zeros((0, 3), np.float32), np.zeros(0, np.int32)
    return np.concatenate(pts).astype(np.float32), np.concatenate(face)


def nearest(query, target, r_max):
    """Brute force over all pairs in float32 -> (dist float32 [n], index int32 [n])."""
    q, t = np.asarray(query, np.float32).reshape(-1, 3), np.asarray(target, np.float32).reshape(-1, 3)
    r_max = np.float32(r_max)
    r2 = np.float32(r_max * r_max)
    n, m = len(q), len(t)
    index = np.full(n, -1, np.int32)
    dist = np.full(n, r_max, np.float32)
    if m == 0 or n == 0:
        return dist, index
    t_ok = np.isfinite(t).all(axis=1)
    with np.errstate(all="ignore"):
        for lo in range(0, n, 512):
            qq = q[lo:lo + 512]
            ex, ey, ez = (qq[:, None, k] - t[None, :, k] for k in range(3))
            d2 = ((ex * ex + ey * ey) + ez * ez).astype(np.float32)
            ok = t_ok[None, :] & np.isfinite(qq).all(axis=1)[:, None] & (d2 <= r2)
            d2 = np.where(ok, d2, np.float32(np.inf))
            j = d2.argmin(axis=1)                                    # the first of equal minima: the lowest index
            best = d2[np.arange(len(qq)), j]
            found = np.isfinite(best)
            index[lo:lo + 512] = np.where(found, j, -1)
            dist[lo:lo + 512] = np.where(found, np.sqrt(best, dtype=np.float32), r_max)
    return dist, index


def distance_stats(dist, index, thr, m, query=None, query_label=None, target_label=None, n_classes=0):
    """-> counts int64 [3], sums float64 [2] (math.fsum: the exact sum rounded once), confusion int64 [C,C] or None."""
    dist, index = np.asarray(dist, np.float32), np.asarray(index, np.int64)
    counting = np.ones(len(dist), bool) if query is None else np.isfinite(np.asarray(query, np.float32).reshape(-1, 3)).all(axis=1)
    found = counting & (index >= 0) & (index < m)
    within = found & (dist <= np.float32(thr))
    counts = np.array([counting.sum(), found.sum(), within.sum()], np.int64)
    sums = np.array([math.fsum(dist[counting].astype(np.float64)), math.fsum(dist[found].astype(np.float64))], np.float64)
    confusion = None
    if n_classes:
        confusion = np.zeros((n_classes, n_classes), np.int64)
        a = np.asarray(query_label, np.int64)[within]
        b = np.asarray(target_label, np.int64)[index[within]]
        ok = (a >= 0) & (a < n_classes) & (b >= 0) & (b < n_classes)
        np.add.at(confusion, (a[ok], b[ok]), 1)
    return counts, sums, confusion


def quality(pred_points, gt_points, threshold, r_max):
    """accuracy, completion, completion ratio of two clouds by the definitions above (float64 means of the truncated distances)."""
    d_pg, i_pg = nearest(pred_points, gt_points, r_max)
    d_gp, i_gp = nearest(gt_points, pred_points, r_max)
    c_pg, s_pg, _ = distance_stats(d_pg, i_pg, threshold, len(gt_points), pred_points)
    c_gp, s_gp, _ = distance_stats(d_gp, i_gp, threshold, len(pred_points), gt_points)
    return {"accuracy": s_pg[0] / c_pg[0], "completion": s_gp[0] / c_gp[0], "completion_ratio": c_gp[2] / c_gp[0], "precision": c_pg[2] / c_pg[0]}
