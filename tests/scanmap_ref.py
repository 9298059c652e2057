"""A numpy restatement, in our own words, of what csrc/scanmap.hip computes (include/mi355nerf.h, "planner cost map"): the scan update of the
cost map and visit counts as a plain loop over views and beams, the closed form of a Bresenham column, the skip policy, vm, the goal
list and the goal pick.  tests/test_scanmap_cpu.py holds it to the reference's own answers (tests/golden/scan_maps.npz); the GPU tests
compare the kernels with it exactly."""
import numpy as np

TWO_PI = 2 * np.pi
FAR = 1 << 30
MAX_BORDERED_CELLS = 40000
UNREACHED = 0xFFFFFFFF
COST_OF_CODE = np.array([0.5, 0.0, 1.0])


def state_bytes(nx, nz):
    if nx <= 0 or nz <= 0 or (nx + 2) * (nz + 2) > MAX_BORDERED_CELLS:
        return 0
    return 3 * nx * nz * 4


def align_angles(width):
    half = width // 2
    ramp = (np.arange(half) + 0.5) / half
    return np.concatenate([np.arctan(ramp)[::-1], np.arctan(-ramp)])


def yaw_of(poses):
    m = np.asarray(poses, np.float64).reshape(-1, 4, 4)
    return np.arctan2(m[:, 0, 2], m[:, 0, 0])


def centre_of(poses, aabb, res):
    m = np.asarray(poses, np.float64).reshape(-1, 4, 4)
    g = (m[:, :3, 3] - np.asarray(aabb)[:3]) // res
    return g[:, [0, 2]].astype(np.int64)


def end_coordinates(depth_row, align, yaw, loc, aabb, res):
    """The float64 grid coordinates (before rounding) of the end of every beam of one view."""
    d = np.asarray(depth_row).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        a = (np.asarray(align, np.float64) + yaw) % TWO_PI
        ox = np.sin(-a) * d + loc[0]
        oy = -np.cos(-a) * d + loc[1]
        return (ox - aabb[2]) / res, (oy - aabb[0]) / res


def settle_depths(depth_rows, align, yaws, locs, aabb, res, margin=1e-6):
    """A copy of float32 `depth_rows` [V,W] in which every finite depth whose end coordinate lies within `margin` of a half-integer has
    been moved (by a part in 10^4 at a time), so that a last-bit difference between two sin / cos cannot move an end cell."""
    out = np.array(depth_rows, np.float32, copy=True)
    for v in range(out.shape[0]):
        for _ in range(64):
            fx, fy = end_coordinates(out[v], align, yaws[v], locs[v], aabb, res)
            with np.errstate(invalid="ignore"):
                close = (np.abs(fx - np.floor(fx) - 0.5) < margin) | (np.abs(fy - np.floor(fy) - 0.5) < margin)
            close &= np.isfinite(out[v]) & (np.abs(fx) < 1e6) & (np.abs(fy) < 1e6)       # far beams are skipped whatever their last bit
            if not close.any():
                break
            out[v, close] = out[v, close] * np.float32(1.0001) + np.float32(1e-4)
        else:
            raise AssertionError("a depth would not move away from a half-integer")
    return out


def column_y(x1, y1, x2, y2, k):
    """The y of column k (k may be an array) of the walk whose ends, after the steep and end swaps, are (x1, y1), (x2, y2), x1 <= x2: the
    error term starts at dx // 2, loses |dy| per column and gains dx whenever it has gone negative, so it stays in [0, dx) and the steps
    taken before column k are the ceiling of (k |dy| - dx // 2) / dx."""
    dx, ady = x2 - x1, abs(y2 - y1)
    k = np.asarray(k, np.int64)
    if dx == 0:
        return np.full(k.shape, y1, np.int64)
    steps = (k * ady - dx // 2 + dx - 1) // dx
    return y1 + (1 if y1 < y2 else -1) * steps


def _oriented(start, end):
    x1, y1, x2, y2 = int(start[0]), int(start[1]), int(end[0]), int(end[1])
    steep = abs(y2 - y1) > abs(x2 - x1)
    if steep:
        x1, y1, x2, y2 = y1, x1, y2, x2
    if x1 > x2:
        x1, y1, x2, y2 = x2, y2, x1, y1
    return steep, x1, y1, x2, y2


def walk_loop(start, end):
    """Every cell of the line from `start` to `end`, by the running error term: int64 [n,2], from the low end of the major axis."""
    steep, x1, y1, x2, y2 = _oriented(start, end)
    dx, ady = x2 - x1, abs(y2 - y1)
    err, y, up = dx // 2, y1, (1 if y1 < y2 else -1)
    cells = []
    for x in range(x1, x2 + 1):
        cells.append((y, x) if steep else (x, y))
        err -= ady
        if err < 0:
            y += up
            err += dx
    return np.array(cells, np.int64).reshape(-1, 2)


def walk_closed(start, end, shape=None):
    """The same cells by the closed form of a column; with `shape` only the columns inside the grid are formed (work bounded by the
    grid), and of those the cells inside it are returned."""
    steep, x1, y1, x2, y2 = _oriented(start, end)
    k_lo, k_hi = 0, x2 - x1
    if shape is not None:
        n_major = shape[1] if steep else shape[0]
        k_lo, k_hi = max(0, -x1), min(k_hi, n_major - 1 - x1)
    if k_hi < k_lo:
        return np.zeros((0, 2), np.int64)
    k = np.arange(k_lo, k_hi + 1, dtype=np.int64)
    x, y = x1 + k, column_y(x1, y1, x2, y2, k)
    cells = np.stack([y, x] if steep else [x, y], axis=1)
    if shape is not None:
        cells = cells[(cells[:, 0] >= 0) & (cells[:, 0] < shape[0]) & (cells[:, 1] >= 0) & (cells[:, 1] < shape[1])]
    return cells


def scan_view(shape, depth_row, align, yaw, loc, centre, aabb, res, info, use_loop=False):
    """One view's plane: int8 [nx,nz], -1 untouched, 0 free, 1 occupied; beams in order, the later write wins.  `info` [4] is added to:
    beams with a negative cell, with a non-finite depth, beyond +-2^30, drawn."""
    nx, nz = shape
    plane = np.full(shape, -1, np.int8)
    fx, fy = end_coordinates(depth_row, align, yaw, loc, aabb, res)
    cx, cy = int(centre[0]), int(centre[1])
    for j in range(len(fx)):
        if not np.isfinite(np.float64(depth_row[j])):
            info[1] += 1
            continue
        rx, ry = np.rint(fx[j]), np.rint(fy[j])                                        # round-half-even
        if not (abs(rx) <= FAR and abs(ry) <= FAR) or abs(cx) > FAR or abs(cy) > FAR:
            info[2] += 1
            continue
        ix, iy = int(rx), int(ry)
        info[3] += 1
        if min(ix, iy, cx, cy) < 0:
            info[0] += 1
        if use_loop:
            cells = walk_loop((cx, cy), (ix, iy))
            cells = cells[(cells[:, 0] >= 0) & (cells[:, 0] < nx) & (cells[:, 1] >= 0) & (cells[:, 1] < nz)]
        else:
            cells = walk_closed((cx, cy), (ix, iy), shape)
        plane[cells[:, 0], cells[:, 1]] = 0
        for px, py in ((ix, iy), (ix + 1, iy), (ix, iy + 1), (ix + 1, iy + 1)):
            if 0 <= px < nx and 0 <= py < nz:
                plane[px, py] = 1
    return plane


def scan_update(codes, visits, depth_rows, align, yaws, locs, centres, aabb, res, info=None, use_loop=False, after_each=None):
    """Fold views into `codes` (int32 [nx,nz]: 0 unknown, 1 free, 2 occupied) and `visits` (int32 [nx,nz]) in place, view after view."""
    info = np.zeros(4, np.int64) if info is None else info
    for v in range(len(yaws)):
        plane = scan_view(codes.shape, depth_rows[v], align, yaws[v], locs[v], centres[v], aabb, res, info, use_loop)
        codes[plane == 1] = 2
        codes[plane == 0] = 1
        visits[plane == 0] += 1
        if after_each is not None:
            after_each(v, codes, visits)
    return info


def cost_map(codes):
    return COST_OF_CODE[codes]


def vm_of(blocked, visits):
    """float64 [nx,nz]: -1 on blocked cells (value above 0), exp(-(visits - least) / 5) on the others, least taken over those."""
    free = ~(np.asarray(blocked) > 0)
    vm = np.full(free.shape, -1.0)
    if free.any():
        v = np.asarray(visits)[free].astype(np.float64)
        vm[free] = np.exp(-(v - v.min()) / 5)
    return vm


def goal_list(vm, field=None):
    """int32 [n,2]: the cells with vm >= 0 that `field` (uint32 labels, or None) reaches, in row-major order."""
    keep = vm >= 0
    if field is not None:
        keep &= (np.asarray(field).astype(np.int64) & 0xFFFFFFFF) != UNREACHED
    return np.argwhere(keep).astype(np.int32)


def padded_goal_list(vm, field=None):
    cells = goal_list(vm, field)
    out = np.full((vm.size, 2), -1, np.int32)
    out[:len(cells)] = cells
    return out, len(cells)


def pick(cells, n, u):
    u = np.asarray(u, np.float64)
    if n == 0:
        return np.full((len(u), 2), -1, np.int32)
    k = np.minimum(np.floor(u * n).astype(np.int64), n - 1)
    return cells[k]
