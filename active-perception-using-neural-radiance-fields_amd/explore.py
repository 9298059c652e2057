"""The exploration map of scripts/eval/frontier_baseline.py on the device (csrc/explore.hip): every pixel of a depth image ray-cast through
a voxel grid (:170), which then says where space has been seen free, seen occupied or not seen at all; its top-down view (:188), the
frontier cells of that view (find_frontiers, :52-67), their clusters and the member nearest to the current pose of each (:191-214).  The
same map gives explored volume per planning step, for the stored depth images (what was observed) or for depths rendered by the field
(what the model believes).  The definition is in include/mi355nerf.h ("exploration map") and DESIGN.md."""
import numpy as np
import torch

from . import _lib as L
from . import render as RD
from .voxelmap import VoxelBitMap


class ExplorationMap(VoxelBitMap):
    """A persistent bit grid uint32 [2, words] over the voxels of `aabb`: plane 0 "a ray passed through", plane 1 "a ray ended here".
    Inserts accumulate over the steps of a run and do not depend on the order of the pixels.  Depths beyond `max_range` (and +inf)
    carve free space out to `max_range` and mark nothing occupied."""

    def __init__(self, aabb, voxel_size=0.1, max_range=10.0, device="cuda:0"):
        super().__init__(aabb, voxel_size, 2, lambda res: L.load_library().mnf_explore_map_bytes(*res), device)
        self.max_range = float(np.float32(max_range))

    # ------------------------------------------------------------------ insert
    @torch.no_grad()
    def insert(self, rays_o, rays_d, depth, acc=None, min_depth=0.0, min_acc=0.0, stats=None):
        """Ray-cast pixels into the map: rays_o / rays_d [..., 3], depth [...] (distance along the ray), optionally acc [...]; device
        tensors, one launch, no host copy, no synchronisation.  A pixel is skipped when its depth is NaN or <= min_depth, acc < min_acc,
        or its ray is not finite.  `stats`: an int64 device tensor [2] to which {voxel steps, atomic ORs} are added (measurements)."""
        L.require_gpu(rays_o, rays_d, depth, acc, stats)
        o, d, dep, a, n = self._flat_rays(rays_o, rays_d, depth, acc)
        if stats is not None and (stats.dtype != torch.int64 or stats.numel() != 2 or not stats.is_contiguous()):
            raise TypeError("stats is a contiguous int64 tensor of two elements")
        L.launch(L.load_library().mnf_explore_map_insert, L.ptr(self.bits), *self.resolution, self._gmin, self.voxel_size, self.max_range, L.ptr(o),
                 L.ptr(d), L.ptr(dep), L.ptr(a), n, float(min_depth), float(min_acc), L.ptr(stats))

    @torch.no_grad()
    def insert_views(self, radiance_field, estimator, poses, width, height, focal, near_plane, render_step_size, scale, cone_angle, alpha_thre,
                     **insert_kw):
        """The map of what the field believes: `poses` are rendered exactly as `SemanticObjectMap.insert_views` renders them (the same
        rays, the same `render_views` call, background zeros) and the finished depth and acc planes go straight into `insert` with the
        rays that made them.  Returns the render's dict of device tensors."""
        o, d, r = self._render_poses(radiance_field, estimator, poses, width, height, focal, near_plane, render_step_size, scale, cone_angle, alpha_thre)
        self.insert(o, d, r["depth"], acc=r["acc"], **insert_kw)
        return r

    @torch.no_grad()
    def insert_dataset(self, dataset, image_ids, depth_along="z", **insert_kw):
        """The map of what was observed (the reference's own use): the stored depth images of views `image_ids` of a `Dataset`, either
        storage layout, with rays from `generate_image_rays` on the dataset's poses and K.  `depth_along` as in
        `SemanticObjectMap.insert_dataset`: "z" turns Habitat's planar depth into the ray length, "ray" takes it as stored."""
        got = self._dataset_rays(dataset, image_ids, depth_along)
        if got is not None:
            self.insert(got[1].origins, got[1].viewdirs, got[2], **insert_kw)

    # ------------------------------------------------------------------ read-outs
    @torch.no_grad()
    def counts_device(self):
        """{free, occupied, unknown} voxels: int64 device tensor [3]; does not synchronise."""
        counts = torch.empty(3, dtype=torch.int64, device=self.device)
        L.launch(L.load_library().mnf_explore_map_count, L.ptr(self.bits), *self.resolution, L.ptr(counts))
        return counts

    def counts(self):
        """dict(free, occupied, unknown, explored_volume): the voxel counts and (free + occupied) * voxel_size^3 in float64."""
        free, occupied, unknown = (int(v) for v in self.counts_device().cpu().numpy())
        return {"free": free, "occupied": occupied, "unknown": unknown, "explored_volume": float(free + occupied) * float(self.voxel_size) ** 3}

    def _layers(self, y_lo, y_hi):
        Y = self.resolution[1]
        y_lo, y_hi = 0 if y_lo is None else int(y_lo), Y if y_hi is None else int(y_hi)
        if not 0 <= y_lo <= y_hi <= Y:
            raise ValueError(f"layers [{y_lo}, {y_hi}) outside [0, {Y}]")
        return y_lo, y_hi

    @torch.no_grad()
    def top_down(self, y_lo=None, y_hi=None):
        """int8 device tensor [X, Z] over the layers y_lo <= y < y_hi (default: all): 1 where the column slab holds an occupied voxel,
        else 0 where it holds a free one, else -1 (the grid frontier_baseline.py:188 reads).  Does not synchronise."""
        y_lo, y_hi = self._layers(y_lo, y_hi)
        X, _, Z = self.resolution
        grid = torch.empty(X, Z, dtype=torch.int8, device=self.device)
        L.launch(L.load_library().mnf_explore_map_topdown, L.ptr(self.bits), *self.resolution, y_lo, y_hi, L.ptr(grid))
        return grid

    def _frontiers_device(self, grid, max_frontiers):
        X, _, Z = self.resolution
        mf = X * Z if max_frontiers is None else int(max_frontiers)
        dev = self.device
        out = dict(cells=torch.empty(mf, 2, dtype=torch.int32, device=dev), mult=torch.empty(mf, dtype=torch.int32, device=dev),
                   info=torch.empty(2, dtype=torch.int64, device=dev), max_frontiers=mf)
        L.launch(L.load_library().mnf_explore_map_frontiers, L.ptr(grid), X, Z, mf, L.ptr(out["cells"]), L.ptr(out["mult"]), L.ptr(out["info"]))
        return out

    @torch.no_grad()
    def frontiers(self, y_lo=None, y_hi=None, max_frontiers=None):
        """The frontier cells of `top_down(y_lo, y_hi)` on the host: `cells` [F,2] int32 (x, z) in ascending x * Z + z and `mult` [F]
        int32, how often find_frontiers lists each (1 .. 3).  The default capacity, X * Z, cannot overflow."""
        f = self._frontiers_device(self.top_down(y_lo, y_hi), max_frontiers)
        info = f["info"].cpu().numpy()
        if info[1]:
            raise L.MnfError(f"{int(info[0])} frontier cells exceed max_frontiers = {f['max_frontiers']}")
        n = int(info[0])
        return {"cells": f["cells"][:n].cpu().numpy(), "mult": f["mult"][:n].cpu().numpy()}

    def cell_of(self, world_xz):
        """Float64 cell coordinates of a world (x, z): the inverse of a goal's world position, grid_min + (cell + 0.5) * voxel_size."""
        w = np.asarray(world_xz, np.float64).reshape(2)
        return (w - self.grid_min.astype(np.float64)[[0, 2]]) / float(self.voxel_size) - 0.5

    @torch.no_grad()
    def frontier_goals(self, current_world_xz, eps2=1, min_samples=3, weighted=True, y_lo=None, y_hi=None, max_frontiers=None, max_clusters=None):
        """What frontier_baseline.py:188-214 computes: the frontier cells (`cells` [F,2], `mult` [F]), their DBSCAN `labels` [F] (-1:
        noise; `weighted` counts each cell as often as the reference lists it) and per cluster the member nearest to
        `current_world_xz`: `goal_cells` [K,2] int32, `goals` [K,2] float64 world (x, z) = grid_min + (cell + 0.5) * voxel_size, and
        `sizes` [K] int32 member cells.  Everything runs on the device; one small host copy happens at the end."""
        lib = L.load_library()
        dev = self.device
        X, _, Z = self.resolution
        cur = self.cell_of(current_world_xz)
        f = self._frontiers_device(self.top_down(y_lo, y_hi), max_frontiers)
        mf = f["max_frontiers"]
        mc = mf if max_clusters is None else int(max_clusters)
        labels = torch.empty(mf, dtype=torch.int32, device=dev)
        goals = torch.empty(mc, 2, dtype=torch.int32, device=dev)
        sizes = torch.empty(mc, dtype=torch.int32, device=dev)
        info = torch.empty(2, dtype=torch.int64, device=dev)
        nbytes = int(lib.mnf_explore_map_frontier_clusters_workspace_bytes(X, Z, mf, mc))
        if nbytes <= 0:
            raise L.MnfError(f"no clustering workspace for {mf} frontier cells and {mc} clusters")
        with torch.cuda.device(dev):
            ws = RD._workspace((dev, "explore"), nbytes)
            L.launch(lib.mnf_explore_map_frontier_clusters, L.ptr(f["cells"]), L.ptr(f["mult"]), L.ptr(f["info"]), mf, X, Z, int(eps2), int(min_samples),
                     int(bool(weighted)), float(cur[0]), float(cur[1]), mc, L.ptr(labels), L.ptr(goals), L.ptr(sizes), L.ptr(info), L.ptr(ws), nbytes)
        finfo, cinfo = f["info"].cpu().numpy(), info.cpu().numpy()
        if finfo[1] or cinfo[1]:
            raise L.MnfError(f"{int(finfo[0])} frontier cells / {int(cinfo[0])} clusters exceed the capacity ({mf} / {mc})")
        n, k = int(finfo[0]), int(cinfo[0])
        goal_cells = goals[:k].cpu().numpy()
        world = self.grid_min.astype(np.float64)[[0, 2]][None] + (goal_cells.astype(np.float64) + 0.5) * float(self.voxel_size)
        return {"cells": f["cells"][:n].cpu().numpy(), "mult": f["mult"][:n].cpu().numpy(), "labels": labels[:n].cpu().numpy(),
                "goal_cells": goal_cells, "goals": world, "sizes": sizes[:k].cpu().numpy()}

    @torch.no_grad()
    def goal_paths(self, current_world_xz, goal_cells, y_lo=None, y_hi=None, unknown_blocked=True):
        """The way to each of `goal_cells` [K,2] (x, z), e.g. `frontier_goals`' "goal_cells", over `top_down(y_lo, y_hi)`: occupied cells
        are blocked, unknown cells too when `unknown_blocked`; moves and costs are the planner's (apnrf_amd.planning).  The source is the
        cell floor(cell_of(current) + 0.5).  One shortest-path field, one trace.  -> `lengths_m` float64 [K] = (a + b sqrt(2)) *
        voxel_size, inf where a goal cannot be reached; `paths` int32 [total,2] cells, goal first, packed at `offsets` int64 [K+1]
        (host arrays).  The frontier baseline can order its goals by the way to them instead of the straight line."""
        from . import planning as PL
        grid = self.top_down(y_lo, y_hi)
        blocked = ((grid == 1) | (grid == -1)) if unknown_blocked else (grid == 1)
        cur = np.floor(self.cell_of(current_world_xz) + 0.5)
        big = float(1 << 30)
        source = torch.tensor([[int(min(max(cur[0], -1.0), big)), int(min(max(cur[1], -1.0), big))]], dtype=torch.int32, device=self.device)
        out = PL.path_field(blocked.to(torch.int32), source)
        PL.check_info(out["info"])
        cells = np.asarray(goal_cells, np.int64).reshape(-1, 2)
        goals = torch.from_numpy(np.concatenate([np.zeros((cells.shape[0], 1), np.int64), cells], axis=1).astype(np.int32)).to(self.device)
        t = PL.trace_paths(out["field"], goals)
        X, _, Z = self.resolution
        gx, gz = goals[:, 1].long(), goals[:, 2].long()
        inside = (gx >= 0) & (gx < X) & (gz >= 0) & (gz < Z)
        cost = PL.field_costs(out["field"][0])[gx.clamp(0, X - 1), gz.clamp(0, Z - 1)]
        cost = torch.where(inside, cost, torch.full_like(cost, float("inf")))
        return {"lengths_m": cost.cpu().numpy() * float(self.voxel_size), "paths": t["paths"].cpu().numpy(), "offsets": t["offsets"].cpu().numpy()}


def next_goal(goals, goal_cells, current_world_xz, visited):
    """The host glue of frontier_baseline.py:210-223 on the tiny goal arrays: drop the goals whose cell is in `visited` (a list of
    (x, z) cells the caller keeps), order the rest by distance to the current position, nearest first, and append the winner's cell
    to `visited`.  -> (world (x, z) [2] float64, order [K'] int64 of the goals that remain), or (None, empty) when none is left."""
    goal_cells = np.asarray(goal_cells).reshape(-1, 2)
    seen = {(int(x), int(z)) for x, z in visited}
    left = np.array([i for i, c in enumerate(goal_cells) if (int(c[0]), int(c[1])) not in seen], np.int64)
    if left.size == 0:
        return None, left
    g = np.asarray(goals, np.float64).reshape(-1, 2)[left]
    order = left[np.argsort(np.linalg.norm(g - np.asarray(current_world_xz, np.float64).reshape(1, 2), axis=1), kind="stable")]
    visited.append((int(goal_cells[order[0], 0]), int(goal_cells[order[0], 1])))
    return np.asarray(goals, np.float64).reshape(-1, 2)[order[0]].copy(), order
