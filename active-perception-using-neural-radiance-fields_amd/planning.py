"""The planner's grid search on the device (csrc/planning.hip): `Dijkstra(aabb, path_finding_map, voxel_grid_size, 0.05).planning(...)` of
planning/dijkstra.py, which sample_traj (planning/planning_funcs.py:288-326) calls once per sampled goal, as one single-source
shortest-path field per start cell and paths traced out of it.  A field answers every goal from its start: reached or not, at what
cost, along which cells.  The definition (moves, exact integer labels, the trace rule) is in include/mi355nerf.h ("planner grid search")
and DESIGN.md.

Further down, the planner's cost map and goal draw (csrc/scanmap.hip): `ScanCostMap` for `update_cost_map`
(planning/planning_funcs.py:192-219) and the maps it updates, `goal_cells` for the vm map and free cells of sample_traj (:262-298),
`draw_goals` for its draw-and-reject loop (:296-326); include/mi355nerf.h ("planner cost map")."""
import ctypes
import math

import numpy as np
import torch

from . import _lib as L

UNREACHED = -1          # 0xFFFFFFFF viewed as int32
SQRT2 = math.sqrt(2.0)


def _device_int32(a, device):
    t = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(np.asarray(a)))
    if device is not None:
        t = t.to(device)
    L.require_gpu(t)
    return L.contig(t, torch.int32)


@torch.no_grad()
def path_field(blocked, sources, limits=None):
    """Shortest-path fields.  `blocked` [nx,ny] or [B,nx,ny] (non-zero = obstacle; `mnf_planner_map`'s int32 output as it stands),
    `sources` [B,2] integer cells (x, y), `limits` (lim_x, lim_y) or None for (nx, ny).  -> {"field": int32 [B,nx,ny] holding the
    uint32 labels (a << 16) | b, -1 = not reached, "info": int64 [B,2] = {reached cells, sweeps}; info[b,0] == -1 reports a field
    that hit the sweep cap (`check_info`)}.  Device tensors; one launch, no host copy, no synchronisation."""
    blocked = blocked if torch.is_tensor(blocked) else torch.from_numpy(np.ascontiguousarray(np.asarray(blocked)))
    L.require_gpu(blocked)
    dev = blocked.device
    if blocked.dim() not in (2, 3):
        raise ValueError(f"blocked is [nx,ny] or [B,nx,ny] (got {tuple(blocked.shape)})")
    if blocked.dtype != torch.int32:
        blocked = (blocked != 0).to(torch.int32)
    blocked = blocked.contiguous()
    src = _device_int32(sources, dev).reshape(-1, 2)
    B = int(src.shape[0])
    n_maps = 1 if blocked.dim() == 2 else int(blocked.shape[0])
    nx, ny = int(blocked.shape[-2]), int(blocked.shape[-1])
    if n_maps != 1 and n_maps != B:
        raise ValueError(f"{n_maps} maps for {B} sources: one map, or one per source")
    lim_x, lim_y = (nx, ny) if limits is None else (int(limits[0]), int(limits[1]))
    lib = L.load_library()
    if nx <= 0 or ny <= 0 or (B > 0 and int(lib.mnf_path_field_bytes(nx, ny, B)) <= 0):
        raise L.MnfError(f"a {nx} x {ny} map is outside what a path field holds: (nx + 2)(ny + 2) <= 40000")
    field = torch.empty(B, nx, ny, dtype=torch.int32, device=dev)
    info = torch.empty(B, 2, dtype=torch.int64, device=dev)
    L.launch(lib.mnf_path_field, L.ptr(blocked), n_maps, nx, ny, lim_x, lim_y, L.ptr(src), B, L.ptr(field), L.ptr(info))
    return {"field": field, "info": info}


def check_info(info):
    """Raise if a field of `path_field` ended at the sweep cap instead of a fixpoint (one host copy)."""
    bad = (info.reshape(-1, 2)[:, 0] < 0).nonzero().reshape(-1).cpu().numpy()
    if bad.size:
        raise L.MnfError(f"path field {bad.tolist()}: no fixpoint within nx * ny sweeps (a logic error; the field is not usable)")


def field_labels(field):
    """(a, b, reached): the straight and diagonal move counts as int64 and the reached mask of a field."""
    u = field.to(torch.int64) & 0xFFFFFFFF
    return u >> 16, u & 0xFFFF, field != UNREACHED


def field_costs(field):
    """float64 a + b * sqrt(2), formed freshly from the two integers of every label; inf where a cell is not reached."""
    a, b, reached = field_labels(field)
    diag = b.to(torch.float64) * SQRT2
    cost = a.to(torch.float64) + diag
    return torch.where(reached, cost, torch.full_like(cost, float("inf")))


@torch.no_grad()
def trace_paths(field, goals):
    """The paths of `goals` [G,3] = {field index, x, y} through `field` [B,nx,ny] (or [nx,ny]): `paths` int32 [total,2] cells, goal first
    and source last, packed at `offsets` int64 [G+1]; `lengths` int64 [G] = a + b + 1, or 0 for a goal that is not reached or lies
    outside.  Device tensors.  The labels of the goals are gathered with torch, lengths and offsets are formed on the device, and the
    total is the one host read."""
    L.require_gpu(field)
    if field.dtype != torch.int32:
        raise TypeError("field is the int32 tensor path_field returns")
    field = field.contiguous()
    if field.dim() == 2:
        field = field[None]
    dev = field.device
    B, nx, ny = (int(v) for v in field.shape)
    g = _device_int32(goals, dev).reshape(-1, 3)
    G = int(g.shape[0])
    f, x, y = g[:, 0].long(), g[:, 1].long(), g[:, 2].long()
    inside = (f >= 0) & (f < B) & (x >= 0) & (x < nx) & (y >= 0) & (y < ny)
    lab = field[f.clamp(0, B - 1), x.clamp(0, nx - 1), y.clamp(0, ny - 1)]
    a, b, reached = field_labels(lab)
    lengths = torch.where(inside & reached, a + b + 1, torch.zeros_like(a))
    offsets = torch.zeros(G + 1, dtype=torch.int64, device=dev)
    offsets[1:] = torch.cumsum(lengths, 0)
    total = int(offsets[-1].item()) if G else 0
    paths = torch.empty(max(total, 1), 2, dtype=torch.int32, device=dev)                # never a null pointer, also when no goal is reached
    info = torch.empty(2, dtype=torch.int64, device=dev)
    L.launch(L.load_library().mnf_path_trace, L.ptr(field), B, nx, ny, L.ptr(g), L.ptr(offsets), G, L.ptr(paths), L.ptr(info))
    return {"paths": paths[:total], "offsets": offsets, "lengths": lengths, "info": info}


class Dijkstra:
    """planning/dijkstra.py's class on the device: the same constructor and attributes, `planning(sx, sy, gx, gy)` with the same
    result type.  `from apnrf_amd.planning import Dijkstra` replaces `from dijkstra import Dijkstra`.  The map is copied to the device
    once, at construction.  The field of a start cell is cached, so further goals from the same start cost one trace each
    (`planning`) or one trace for all of them (`planning_many`), and `reachable(sx, sy)` says which goals are worth drawing.
    Paths have the reference's cost and make-up; of several equal ones the reference's own choice follows the insertion order of a
    Python dict and need not be this one.  The one documented difference: a start outside the map gives None for every goal."""

    def __init__(self, aabb, planning_map, resolution, robot_radius, device="cuda:0"):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise L.MnfError("the grid search runs on a GPU; there is no CPU fallback")
        if not resolution > 0:
            raise ValueError(f"resolution must be positive (got {resolution})")
        self.resolution = resolution
        self.robot_radius = robot_radius
        self.min_x = 0
        self.min_y = 0
        self.max_x = aabb[3] - aabb[0]
        self.max_y = aabb[4] - aabb[1]
        self.x_width = int(planning_map.shape[0])
        self.y_width = int(planning_map.shape[1])
        self.obstacle_map = planning_map
        self.motion = self.get_motion_model()
        m = planning_map if torch.is_tensor(planning_map) else torch.from_numpy(np.ascontiguousarray(np.asarray(planning_map)))
        self.blocked = (m.to(self.device) != 0).to(torch.int32).contiguous()
        # verify_node: px = i * resolution + min < max, evaluated as the reference evaluates it; the positions ascend, so a count is a limit
        self.lim_x = sum(1 for i in range(self.x_width) if i * self.resolution + self.min_x < self.max_x)
        self.lim_y = sum(1 for i in range(self.y_width) if i * self.resolution + self.min_y < self.max_y)
        self._fields = {}
        self.fields_computed = 0

    @staticmethod
    def get_motion_model():
        return [[1, 0, 1], [0, 1, 1], [-1, 0, 1], [0, -1, 1], [-1, -1, SQRT2], [-1, 1, SQRT2], [1, -1, SQRT2], [1, 1, SQRT2]]

    def calc_position(self, index, minp):
        return index * self.resolution + minp

    def calc_xy_index(self, position, minp):
        return round((position - minp) / self.resolution)

    def clear_cache(self):
        self._fields.clear()

    def _field(self, sx, sy):
        """The cached field [nx,ny] of the start's cell, or None for a start outside the map."""
        cell = (int(self.calc_xy_index(sx, self.min_x)), int(self.calc_xy_index(sy, self.min_y)))
        if not (0 <= cell[0] < self.x_width and 0 <= cell[1] < self.y_width):
            return None
        if cell not in self._fields:
            out = path_field(self.blocked, torch.tensor([cell], dtype=torch.int32, device=self.device), (self.lim_x, self.lim_y))
            check_info(out["info"])
            self._fields[cell] = out["field"][0]
            self.fields_computed += 1
        return self._fields[cell]

    def planning_many(self, sx, sy, goals_xy):
        """One trace launch for all `goals_xy` [(gx, gy), ...] from one start -> a list of (rx, ry) | None."""
        goals_xy = list(goals_xy)
        field = self._field(sx, sy)
        if field is None or not goals_xy:
            return [None] * len(goals_xy)
        cells = [(0, int(self.calc_xy_index(gx, self.min_x)), int(self.calc_xy_index(gy, self.min_y))) for gx, gy in goals_xy]
        big = 1 << 30                                                                  # any index beyond it lies outside every map
        cells = [(f, max(-1, min(x, big)), max(-1, min(y, big))) for f, x, y in cells]
        t = trace_paths(field, torch.tensor(cells, dtype=torch.int32, device=self.device))
        paths, offsets, info = t["paths"].cpu().numpy(), t["offsets"].cpu().numpy(), t["info"].cpu().numpy()
        if info[1]:
            raise L.MnfError(f"{int(info[1])} paths did not fit their slots")
        out = []
        for g in range(len(cells)):
            p = paths[offsets[g]:offsets[g + 1]]
            if p.shape[0] == 0:
                out.append(None)
                continue
            out.append(([self.calc_position(int(i), self.min_x) for i in p[:, 0]], [self.calc_position(int(i), self.min_y) for i in p[:, 1]]))
        return out

    def planning(self, sx, sy, gx, gy):
        """(rx, ry): Python lists of index * resolution + min, goal first and start last; None where the goal is not reached."""
        return self.planning_many(sx, sy, [(gx, gy)])[0]

    def reachable(self, sx, sy):
        """bool device tensor [nx,ny]: the cells `planning` finds a path to from this start."""
        field = self._field(sx, sy)
        if field is None:
            return torch.zeros(self.x_width, self.y_width, dtype=torch.bool, device=self.device)
        return field != UNREACHED

    def costs(self, sx, sy):
        """float64 device tensor [nx,ny]: the path cost in cells (times `resolution` for metres), inf where not reached."""
        field = self._field(sx, sy)
        if field is None:
            return torch.full((self.x_width, self.y_width), float("inf"), dtype=torch.float64, device=self.device)
        return field_costs(field)


# ---------------------------------------------------------------------- the cost map and the goal draw (csrc/scanmap.hip)
COST_VALUES = (0.5, 0.0, 1.0)          # the cost codes 0 unknown, 1 free, 2 occupied as the reference's cost_map holds them
DECAY_ENTRIES = 3728                   # np.exp(-m / 5) is 0.0 from m = 3727 on


def align_angles(width):
    """The angle of every image column from the optical axis (scripts/pipeline.py:227-230 for 640 columns) for any even width."""
    width = int(width)
    if width <= 0 or width % 2:
        raise ValueError(f"align_angles is defined for an even, positive width (got {width}); pass align_angles= for another scan")
    half = width // 2
    r = np.arctan(np.linspace(0.5, half - 0.5, half) / half).tolist()
    r.reverse()
    l = np.arctan(-np.linspace(0.5, half - 0.5, half) / half).tolist()
    return np.array(r + l)


def yaw_of(poses_c2w):
    """float64 [V]: the first angle of scipy's `Rotation.from_matrix(R).as_euler("yzx")` (scripts/pipeline.py:275) in closed form.  The
    extrinsic sequence y, z, x composes to R = Rx(c) Rz(b) Ry(a), whose first row is (cos b cos a, -sin b, cos b sin a); away from the
    singularity cos b = 0 that makes a = atan2(R[0,2], R[0,0])."""
    m = np.asarray(poses_c2w, np.float64)
    m = m.reshape((-1,) + m.shape[-2:])
    return np.arctan2(m[:, 0, 2], m[:, 0, 0])


def _decay_table():
    return np.exp(-np.arange(DECAY_ENTRIES, dtype=np.float64) / 5)


class ScanCostMap:
    """`cost_map` and `visiting_map` of scripts/pipeline.py:122-125 on the device, and the loops over `update_cost_map`
    (planning/planning_funcs.py:192-219) at pipeline.py:272-292, :1115-1138 and :1171-1189 as one call per batch of views.  The grid is
    the reference's (main_grid_resolution[0], main_grid_resolution[2]).  The definition, and the
    one deliberate difference (a cell with a negative index is skipped and counted, not wrapped round), are in include/mi355nerf.h
    ("planner cost map")."""

    def __init__(self, aabb, resolution, device="cuda:0"):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise L.MnfError("ScanCostMap lives on a GPU; there is no CPU fallback")
        if not resolution > 0:
            raise ValueError(f"resolution must be positive (got {resolution})")
        self.aabb = np.asarray(aabb.detach().cpu().numpy() if torch.is_tensor(aabb) else aabb).reshape(6)
        self.resolution = resolution
        a32 = self.aabb.astype(np.float32)                                             # pipeline.py:113-125
        n = ((a32[3:] - a32[:3]) / resolution).astype(int).tolist()
        self.nx, self.nz = int(n[0]), int(n[2])
        nbytes = int(L.load_library().mnf_scan_map_bytes(self.nx, self.nz)) if self.nx > 0 and self.nz > 0 else 0
        if nbytes <= 0:
            raise L.MnfError(f"a {self.nx} x {self.nz} grid is outside what the cost map holds: (nx + 2)(nz + 2) <= 40000")
        self._aabb_c = (ctypes.c_double * 6)(*[float(v) for v in self.aabb])
        self.state = torch.zeros(3, self.nx, self.nz, dtype=torch.int32, device=self.device)   # cost codes, visit counts, scratch
        self._info = torch.zeros(4, dtype=torch.int64, device=self.device)
        self._values = torch.tensor(COST_VALUES, dtype=torch.float64, device=self.device)
        self._align = {}

    def clear(self):
        self.state.zero_()
        self._info.zero_()

    @property
    def codes(self):
        """int32 device tensor [nx,nz]: 0 unknown, 1 free, 2 occupied."""
        return self.state[0]

    @property
    def visits(self):
        """int32 device tensor [nx,nz]: how many views left each cell free (what `goal_cells` takes)."""
        return self.state[1]

    def cost_map(self):
        """float64 device tensor [nx,nz]: the reference's cost_map (0.5 unknown, 0.0 free, 1.0 occupied)."""
        return self._values[self.state[0].long()]

    def visiting_map(self):
        """float64 device tensor [nx,nz]: the reference's self.visiting_map."""
        return self.state[1].to(torch.float64)

    def info(self):
        """dict of beam counts since the last clear(): negative_cell (drawn without those cells), bad_depth, far (both skipped), drawn."""
        v = [int(x) for x in self._info.cpu().numpy()]
        return {"negative_cell": v[0], "bad_depth": v[1], "far": v[2], "drawn": v[3]}

    def view_inputs(self, poses_c2w):
        """(yaw [V], loc [V,2], centre [V,2] int32) on the host, formed as scripts/pipeline.py:274-282 forms them."""
        m = np.asarray(poses_c2w.detach().cpu().numpy() if torch.is_tensor(poses_c2w) else poses_c2w, np.float64)
        m = m.reshape((-1,) + m.shape[-2:])
        yaw = yaw_of(m)
        w_loc = m[:, :3, 3]
        with np.errstate(invalid="ignore", over="ignore"):
            g = (w_loc - self.aabb[:3]) // self.resolution
        far = float((1 << 30) + 1)                                                     # beyond +-2^30 the kernel skips the view's beams
        g = np.where(np.isfinite(g), np.clip(g, -far, far), far)
        return yaw, np.ascontiguousarray(w_loc[:, [0, 2]]), np.ascontiguousarray(g[:, [0, 2]].astype(np.int32))

    def _align_device(self, width, align):
        if align is not None:
            a = align if torch.is_tensor(align) else torch.from_numpy(np.ascontiguousarray(np.asarray(align, np.float64)))
            a = L.contig(a.to(self.device), torch.float64).reshape(-1)
            if int(a.shape[0]) != width:
                raise ValueError(f"{int(a.shape[0])} align angles for {width} columns")
            return a
        if width not in self._align:
            self._align[width] = torch.from_numpy(align_angles(width)).to(self.device)
        return self._align[width]

    @torch.no_grad()
    def update(self, depth_images, poses_c2w, align_angles=None):
        """Fold the middle rows of `depth_images` [V,H,W] (device or host) taken at `poses_c2w` [V,4,4] into the map, in order.  The
        depth goes up once if it is on the host; yaw, location and centre cell of every view go up in one small copy."""
        d = depth_images if torch.is_tensor(depth_images) else torch.from_numpy(np.ascontiguousarray(np.asarray(depth_images)))
        if d.dim() == 2:
            d = d[None]
        if d.dim() != 3:
            raise ValueError(f"depth_images is [V,H,W] (got {tuple(d.shape)})")
        d = L.contig(d.to(self.device), torch.float32)
        V, H, W = (int(v) for v in d.shape)
        yaw, loc, centre = self.view_inputs(poses_c2w)
        if yaw.shape[0] != V:
            raise ValueError(f"{yaw.shape[0]} poses for {V} depth images")
        if V == 0:
            return
        if H <= 0 or W <= 0:
            raise ValueError(f"empty depth images {tuple(d.shape)}")
        align = self._align_device(W, align_angles)
        packed = np.empty(4 * V, np.float64)                                           # yaw | loc | centre (two int32 per float64 slot)
        packed[:V] = yaw
        packed[V:3 * V] = loc.reshape(-1)
        packed[3 * V:].view(np.int32)[:] = centre.reshape(-1)
        p = torch.from_numpy(packed).to(self.device)
        L.launch(L.load_library().mnf_scan_map_update, L.ptr(self.state), self.nx, self.nz, L.ptr(d), V, H, W, L.ptr(align), L.ptr(p[:V]),
                 L.ptr(p[V:3 * V]), L.ptr(p[3 * V:]), self._aabb_c, float(self.resolution), L.ptr(self._info))

    @torch.no_grad()
    def update_dataset(self, dataset, image_ids, align_angles=None):
        """`update` from the stored depth images and poses of views `image_ids` of a `Dataset`, either storage layout."""
        from . import render as RD
        ids = RD._eval_index_tensor(image_ids, self.device, len(dataset), "image_ids")
        if int(ids.shape[0]) == 0:
            return
        L.require_gpu(dataset.depths, dataset.camtoworlds)
        H, W = int(dataset.height), int(dataset.width)
        self.update(dataset.depths[ids].reshape(-1, H, W), dataset.camtoworlds[ids], align_angles=align_angles)


@torch.no_grad()
def goal_cells(blocked, visits, dijkstra=None, start_xy=None):
    """The vm map of sample_traj (planning/planning_funcs.py:262-276) and the goals worth drawing.  `blocked` [nx,nz] (the
    path-finding map, > 0 = blocked) and `visits` [nx,nz] (`ScanCostMap.visits`, or any integer counts) on the device; with a `Dijkstra`
    and its start (`start_xy` = the (sx, sy) given to `planning`) only cells that start reaches are listed.  -> {"vm": float64
    [nx,nz], "cells": int32 [nx*nz,2] in np.argwhere's order, rows from `count` on are -1, "count": int64 [1]}: device tensors, one
    launch, no synchronisation."""
    blocked = blocked if torch.is_tensor(blocked) else torch.from_numpy(np.ascontiguousarray(np.asarray(blocked)))
    visits = visits if torch.is_tensor(visits) else torch.from_numpy(np.ascontiguousarray(np.asarray(visits)))
    L.require_gpu(blocked, visits)
    dev = blocked.device
    if blocked.dim() != 2 or tuple(visits.shape) != tuple(blocked.shape):
        raise ValueError(f"blocked and visits are [nx,nz] (got {tuple(blocked.shape)} and {tuple(visits.shape)})")
    if visits.dtype.is_floating_point:
        visits = visits.round()
    b, v = L.contig(blocked, torch.int32), L.contig(visits, torch.int32)
    nx, nz = int(b.shape[0]), int(b.shape[1])
    if nx <= 0 or nz <= 0 or int(L.load_library().mnf_scan_map_bytes(nx, nz)) <= 0:
        raise L.MnfError(f"a {nx} x {nz} map is outside the planner's cap: (nx + 2)(nz + 2) <= 40000")
    field = None
    if dijkstra is not None:
        if start_xy is None:
            raise ValueError("a Dijkstra needs start_xy = (sx, sy)")
        if (dijkstra.x_width, dijkstra.y_width) != (nx, nz):
            raise ValueError(f"the Dijkstra's map is {dijkstra.x_width} x {dijkstra.y_width}, blocked is {nx} x {nz}")
        field = dijkstra._field(float(start_xy[0]), float(start_xy[1]))
        if field is None:                                                              # a start outside the map reaches nothing
            field = torch.full((nx, nz), UNREACHED, dtype=torch.int32, device=dev)
        field = field.contiguous()
    decay = torch.from_numpy(_decay_table()).to(dev)
    vm = torch.empty(nx, nz, dtype=torch.float64, device=dev)
    cells = torch.empty(nx * nz, 2, dtype=torch.int32, device=dev)
    count = torch.empty(1, dtype=torch.int64, device=dev)
    L.launch(L.load_library().mnf_planner_goal_map, L.ptr(b), L.ptr(v), L.ptr(field), nx, nz, L.ptr(decay), DECAY_ENTRIES, L.ptr(vm), L.ptr(cells),
             L.ptr(count))
    return {"vm": vm, "cells": cells, "count": count}


@torch.no_grad()
def draw_goals(cells, count, u):
    """int32 device tensor [N,2]: cells[min(floor(u * count), count - 1)] for uniforms `u` [N] in [0, 1) from the caller's generator,
    (-1, -1) when there is no goal.  Uniform over the free cells the start reaches: the distribution of the reference's
    draw-and-reject loop (planning_funcs.py:296-326), not its random stream."""
    L.require_gpu(cells, count)
    dev = cells.device
    if cells.dtype != torch.int32 or count.dtype != torch.int64:
        raise TypeError("cells and count are the tensors goal_cells returns")
    u = u if torch.is_tensor(u) else torch.from_numpy(np.ascontiguousarray(np.asarray(u, np.float64)).reshape(-1))
    u = L.contig(u.to(dev), torch.float64).reshape(-1)
    cells = cells.contiguous()
    n = int(u.shape[0])
    goals = torch.empty(n, 2, dtype=torch.int32, device=dev)
    L.launch(L.load_library().mnf_planner_goal_pick, L.ptr(cells), L.ptr(count), int(cells.shape[0]), L.ptr(u), n, L.ptr(goals))
    return goals
