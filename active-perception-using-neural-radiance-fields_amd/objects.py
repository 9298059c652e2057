"""The semantic object map of scripts/eval/eval_pipeline_offline.py on the device (csrc/objmap.hip): one voxel bit plane per class
filled from depth and label images (:119-138), its clusters and their centroids (:26-42) and the greedy match of those to the
ground-truth object positions (:45-70), which gives the "objects detected over planning steps" number.

Voxels are linked on INTEGER offsets (dx^2 + dy^2 + dz^2 <= link_r2, default 4 = the reference's eps of two voxels), so the clusters
are the connected components of that graph: DBSCAN(eps=sqrt(link_r2), min_samples=1) on the integer coordinates, deterministic and
bit-reproducible ("Semantic object map")."""
import numpy as np
import torch

from . import _lib as L
from . import render as RD
from .voxelmap import VoxelBitMap, grid_resolution, planar_to_ray_scale  # noqa: F401  (both functions are part of this module's interface)


class SemanticObjectMap(VoxelBitMap):
    """A persistent bit grid uint32 [C, words] over the voxels of `aabb` (include/mi355nerf.h: mnf_object_map_*).  Inserts accumulate,
    as the reference's grids do over the steps of a run; classes below `first_class` are never inserted (the reference skips label 0)."""

    def __init__(self, aabb, voxel_size=0.1, num_classes=29, first_class=1, device="cuda:0"):
        self.num_classes, self.first_class = int(num_classes), int(first_class)
        if not 0 <= self.first_class < self.num_classes:
            raise ValueError(f"first_class {first_class} outside [0, {num_classes})")
        super().__init__(aabb, voxel_size, self.num_classes, lambda res: L.load_library().mnf_object_map_bytes(self.num_classes, *res), device,
                         what=f"{self.num_classes} classes of ")

    # ------------------------------------------------------------------ insert
    @torch.no_grad()
    def insert(self, rays_o, rays_d, depth, sem=None, labels=None, acc=None, min_depth=0.0, max_depth=float("inf"), min_acc=0.0):
        """OR pixels into the map: rays_o / rays_d [..., 3], depth [...] (distance along the ray) and either `sem` [..., C] logits
        (class = first argmax) or `labels` [...] (int64 or uint8), optionally `acc` [...]; device tensors, no host copy, no
        synchronisation.  A pixel is skipped when its class is < first_class or >= C, its depth is not finite, <= min_depth or
        > max_depth, acc < min_acc, or its point o + depth d falls outside the grid."""
        if (sem is None) == (labels is None):
            raise ValueError("insert takes exactly one of sem (logits) and labels")
        L.require_gpu(rays_o, rays_d, depth, sem, labels, acc)
        o, d, dep, a, n = self._flat_rays(rays_o, rays_d, depth, acc)
        s = lab = None
        if sem is not None:
            if int(sem.shape[-1]) != self.num_classes:
                raise ValueError(f"sem has {int(sem.shape[-1])} classes, the map {self.num_classes}")
            s = L.contig(sem.reshape(-1, self.num_classes), torch.float32)
            if int(s.shape[0]) != n:
                raise ValueError(f"{int(s.shape[0])} logit rows for {n} depths")
        else:
            if labels.dtype not in (torch.int64, torch.uint8):
                raise TypeError("labels are int64 or uint8 (the dataset's two layouts)")
            lab = labels.reshape(-1).contiguous()
            if int(lab.shape[0]) != n:
                raise ValueError(f"{int(lab.shape[0])} labels for {n} depths")
        L.launch(L.load_library().mnf_object_map_insert, L.ptr(self.bits), self.num_classes, *self.resolution, self._gmin, self.voxel_size,
                 self.first_class, L.ptr(o), L.ptr(d), L.ptr(dep), L.ptr(a), L.ptr(s), L.ptr(lab), int(lab is not None and lab.dtype == torch.uint8), n,
                 float(min_depth), float(max_depth), float(min_acc))

    @torch.no_grad()
    def insert_views(self, radiance_field, estimator, poses, width, height, focal, near_plane, render_step_size, scale, cone_angle, alpha_thre,
                     **insert_kw):
        """The map of what the field believes: `poses` are rendered exactly as `render_image_from_pose` renders them (the same rays, the
        same `render_views` call, background zeros) and the finished device planes go straight into `insert` with the rays that made
        them.  Returns the render's dict of device tensors."""
        o, d, r = self._render_poses(radiance_field, estimator, poses, width, height, focal, near_plane, render_step_size, scale, cone_angle, alpha_thre)
        self.insert(o, d, r["depth"], sem=r["sem"], acc=r["acc"], **insert_kw)
        return r

    @torch.no_grad()
    def insert_dataset(self, dataset, image_ids, depth_along="z", **insert_kw):
        """The map of what was observed (the reference's own use): the stored ground-truth depth and label images of views `image_ids`
        of a `Dataset`, either storage layout, with rays from `generate_image_rays` on the dataset's poses and K.  `depth_along="z"`:
        the stored depth is Habitat's planar depth and the ray length is z * |cam|, cam = ((x - W/2 + 0.5) / f, (y - H/2 + 0.5) / f, 1)
        the camera-space direction of the pixel before normalisation; `"ray"`: the stored depth is the ray length."""
        got = self._dataset_rays(dataset, image_ids, depth_along)
        if got is None:
            return
        ids, rays, depth = got
        L.require_gpu(dataset.semantics)
        self.insert(rays.origins, rays.viewdirs, depth, labels=dataset.semantics[ids], **insert_kw)

    # ------------------------------------------------------------------ read-outs
    @torch.no_grad()
    def voxel_counts(self):
        """Set voxels per class: int64 device tensor [C]; does not synchronise."""
        counts = torch.empty(self.num_classes, dtype=torch.int64, device=self.device)
        L.launch(L.load_library().mnf_object_map_count, L.ptr(self.bits), self.num_classes, *self.resolution, L.ptr(counts))
        return counts

    def _clusters_device(self, link_r2, min_cluster_voxels, points, max_voxels=None, max_clusters=None):
        lib = L.load_library()
        if max_voxels is None:
            max_voxels = int(self.voxel_counts().sum().item())                                   # the one small read-back that sizes the workspace
        if max_clusters is None:
            max_clusters = max_voxels
        dev = self.device
        out = dict(clusters=torch.empty(max_clusters, 5, dtype=torch.float64, device=dev),
                   cluster_counts=torch.empty(self.num_classes, dtype=torch.int64, device=dev), info=torch.empty(4, dtype=torch.int64, device=dev),
                   voxel_ids=torch.empty(max_voxels, dtype=torch.int64, device=dev) if points else None,
                   voxel_cluster=torch.empty(max_voxels, dtype=torch.int32, device=dev) if points else None, max_clusters=max_clusters)
        nbytes = int(lib.mnf_object_map_clusters_workspace_bytes(self.num_classes, *self.resolution, max_voxels))
        if nbytes <= 0:
            raise L.MnfError(f"no clustering workspace for {max_voxels} voxels")
        with torch.cuda.device(dev):
            ws = RD._workspace((dev, "objmap"), nbytes)
            L.launch(lib.mnf_object_map_clusters, L.ptr(self.bits), self.num_classes, *self.resolution, self._gmin, self.voxel_size, int(link_r2),
                     int(min_cluster_voxels), max_voxels, max_clusters, L.ptr(out["clusters"]), L.ptr(out["cluster_counts"]), L.ptr(out["info"]),
                     L.ptr(out["voxel_ids"]), L.ptr(out["voxel_cluster"]), L.ptr(ws), nbytes)
        return out

    def _host_clusters(self, dev_out, points):
        info = dev_out["info"].cpu().numpy()
        if info[2] or info[3]:
            raise L.MnfError(f"object map changed while it was clustered: {int(info[0])} voxels / {int(info[1])} clusters exceed the capacity")
        n = int(info[1])
        rows = dev_out["clusters"][:n].cpu().numpy()
        res = {"class": rows[:, 0].astype(np.int64), "count": rows[:, 1].astype(np.int64), "centroid": rows[:, 2:5].copy(),
               "per_class": dev_out["cluster_counts"].cpu().numpy(), "set_voxels": int(info[0])}
        if points:
            nv = int(info[0])
            ids = dev_out["voxel_ids"][:nv].cpu().numpy()
            X, Y, Z = self.resolution
            cls, lin = ids // (X * Y * Z), ids % (X * Y * Z)
            ijk = np.stack([lin // (Y * Z), (lin // Z) % Y, lin % Z], axis=1)
            res["points"] = self.grid_min.astype(np.float64)[None] + (ijk.astype(np.float64) + 0.5) * float(self.voxel_size)
            res["point_voxel"] = ijk
            res["point_class"] = cls
            res["point_cluster"] = dev_out["voxel_cluster"][:nv].cpu().numpy()
        return res

    @torch.no_grad()
    def clusters(self, link_r2=4, min_cluster_voxels=1, points=False):
        """Clusters of the map on the host: `class` [K] int64, `count` [K] int64 (voxels), `centroid` [K,3] float64 (world),
        `per_class` [C] int64, ordered by class and then by the smallest linear voxel index; with `points=True` also the labelled voxel
        cloud `points` [M,3] float64 (voxel centres, world), `point_voxel` [M,3], `point_class` [M], `point_cluster` [M] (row or -1)."""
        return self._host_clusters(self._clusters_device(link_r2, min_cluster_voxels, points), points)

    @torch.no_grad()
    def detect(self, gt_locations, gt_classes, det_dist_thresh=1.0, **cluster_kw):
        """What `update_sem_step` returns: `detected` [C] objects found per class and their `total`, from the greedy match of the
        clusters to the ground-truth objects `gt_locations` [G,3] of classes `gt_classes` [G] (class ids as the map counts them: the
        reference's list i holds class i + 1); plus `match` [K] (the object of each cluster or -1), `gt_match` [G] (the cluster of
        each object or -1) and the clusters themselves."""
        lib = L.load_library()
        dev = self.device
        loc = torch.as_tensor(np.asarray(gt_locations, np.float64).reshape(-1, 3)).to(dev)
        cls = torch.as_tensor(np.asarray(gt_classes, np.int32).reshape(-1)).to(dev)
        G = int(cls.shape[0])
        if int(loc.shape[0]) != G:
            raise ValueError(f"{int(loc.shape[0])} locations for {G} classes")
        d = self._clusters_device(cluster_kw.pop("link_r2", 4), cluster_kw.pop("min_cluster_voxels", 1), cluster_kw.pop("points", False))
        if cluster_kw:
            raise TypeError(f"unknown arguments {sorted(cluster_kw)}")
        mc = d["max_clusters"]
        detected = torch.empty(self.num_classes, dtype=torch.int32, device=dev)
        match = torch.empty(mc, dtype=torch.int32, device=dev)
        gt_match = torch.empty(G, dtype=torch.int32, device=dev)
        L.launch(lib.mnf_object_map_match, L.ptr(d["clusters"]), L.ptr(d["info"]), mc, self.num_classes, L.ptr(loc), L.ptr(cls), G,
                 float(det_dist_thresh), L.ptr(detected), L.ptr(match), L.ptr(gt_match))
        res = self._host_clusters(d, d["voxel_ids"] is not None)
        res["detected"] = detected.cpu().numpy()
        res["total"] = int(res["detected"].sum())
        res["match"] = match[:len(res["class"])].cpu().numpy()
        res["gt_match"] = gt_match.cpu().numpy()
        return res
