"""The planner's grid search on the device (csrc/planning.hip): `Dijkstra(aabb, path_finding_map, voxel_grid_size, 0.05).planning(...)` of
planning/dijkstra.py, which sample_traj (planning/planning_funcs.py:288-326) calls once per sampled goal, as one single-source
shortest-path field per start cell and paths traced out of it.  A field answers every goal from its start: reached or not, at what
cost, along which cells.  The definition (moves, exact integer labels, the trace rule) is in include/mi355nerf.h ("planner grid search")
and DESIGN.md."""
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
