"""Numpy / heapq restatement of the planner grid search (include/mi355nerf.h "planner grid search"; csrc/planning.hip): a Dijkstra with
the exact integer order of the labels, the trace rule, the limits, `field_costs`, and the maps the tests use.  Nothing here adds a
cost move after move: a label is the pair (a, b) and two labels are compared by the sign of da + db sqrt(2) in integers."""
import functools
import heapq
import math

import numpy as np

UNREACHED = np.uint32(0xFFFFFFFF)
MAX_BORDERED = 40000
# the reference's motion order (dijkstra.py:247-260): the first four are straight
MOVES = ((1, 0), (0, 1), (-1, 0), (0, -1), (-1, -1), (-1, 1), (1, -1), (1, 1))


def sign_cost(da, db):
    """The exact sign of da + db sqrt(2) for integers da, db."""
    if da >= 0 and db >= 0:
        return 1 if (da or db) else 0
    if da <= 0 and db <= 0:
        return -1
    # the signs differ: |da| against |db| sqrt(2)  <=>  da^2 against 2 db^2
    big = da * da - 2 * db * db
    assert big != 0
    return (1 if big > 0 else -1) * (1 if da > 0 else -1)


def less(p, q):
    """(a, b) pairs: is a_p + b_p sqrt(2) < a_q + b_q sqrt(2)?"""
    return sign_cost(p[0] - q[0], p[1] - q[1]) < 0


@functools.total_ordering
class Key:
    __slots__ = ("a", "b")

    def __init__(self, a, b):
        self.a, self.b = a, b

    def __eq__(self, o):
        return self.a == o.a and self.b == o.b

    def __lt__(self, o):
        return sign_cost(self.a - o.a, self.b - o.b) < 0


def bytes_of(nx, ny, n_sources):
    if nx <= 0 or ny <= 0 or n_sources < 0 or (nx + 2) * (ny + 2) > MAX_BORDERED:
        return 0
    return nx * ny * n_sources * 4


def limits_of(aabb, shape, resolution):
    """(lim_x, lim_y) as the reference's verify_node compares: i * resolution + 0 < max."""
    max_x, max_y = aabb[3] - aabb[0], aabb[4] - aabb[1]
    return (sum(1 for i in range(shape[0]) if i * resolution + 0 < max_x), sum(1 for i in range(shape[1]) if i * resolution + 0 < max_y))


def path_field(blocked, source, limits=None):
    """uint32 [nx,ny] labels (a << 16) | b of the unique cheapest (a, b) per cell, 0xFFFFFFFF where not reached; reached cell count."""
    blocked = np.asarray(blocked)
    nx, ny = blocked.shape
    lim_x, lim_y = (nx, ny) if limits is None else limits
    field = np.full((nx, ny), UNREACHED, np.uint32)
    sx, sy = int(source[0]), int(source[1])
    if not (0 <= sx < nx and 0 <= sy < ny):
        return field, 0
    best = {(sx, sy): (0, 0)}
    done = set()
    heap = [(Key(0, 0), sx, sy)]
    while heap:
        k, x, y = heapq.heappop(heap)
        if (x, y) in done:
            continue
        done.add((x, y))
        field[x, y] = np.uint32((k.a << 16) | k.b)
        for m, (mx, my) in enumerate(MOVES):
            px, py = x + mx, y + my
            if not (0 <= px < lim_x and 0 <= py < lim_y) or blocked[px, py] or (px, py) in done:
                continue
            cand = (k.a + 1, k.b) if m < 4 else (k.a, k.b + 1)
            if (px, py) not in best or less(cand, best[(px, py)]):
                best[(px, py)] = cand
                heapq.heappush(heap, (Key(*cand), px, py))
    return field, len(done)


def path_fields(blocked, sources, limits=None):
    """[B,nx,ny] fields and [B] reached counts; `blocked` [nx,ny] or [B,nx,ny]."""
    blocked = np.asarray(blocked)
    out = [path_field(blocked if blocked.ndim == 2 else blocked[i], s, limits) for i, s in enumerate(np.asarray(sources).reshape(-1, 2))]
    nx, ny = blocked.shape[-2:]
    return (np.stack([f for f, _ in out]) if out else np.zeros((0, nx, ny), np.uint32)), np.array([n for _, n in out], np.int64)


def split(field):
    f = np.asarray(field).view(np.uint32) if np.asarray(field).dtype == np.int32 else np.asarray(field, np.uint32)
    return (f >> np.uint32(16)).astype(np.int64), (f & np.uint32(0xFFFF)).astype(np.int64), f != UNREACHED


def field_costs(field):
    a, b, reached = split(field)
    cost = a.astype(np.float64) + b.astype(np.float64) * math.sqrt(2.0)
    return np.where(reached, cost, np.inf)


def trace(field, goal):
    """The cells of the goal's path, goal first and source last ([n,2] int32; n = 0: not reached or outside)."""
    field = np.asarray(field, np.uint32)
    nx, ny = field.shape
    x, y = int(goal[0]), int(goal[1])
    if not (0 <= x < nx and 0 <= y < ny) or field[x, y] == UNREACHED:
        return np.zeros((0, 2), np.int32)
    cells = []
    while True:
        cells.append((x, y))
        lab = int(field[x, y])
        if lab == 0:
            break
        a, b = lab >> 16, lab & 0xFFFF
        for m, (mx, my) in enumerate(MOVES):
            px, py = x - mx, y - my
            if not (0 <= px < nx and 0 <= py < ny):
                continue
            if (m < 4 and a == 0) or (m >= 4 and b == 0):
                continue
            want = ((a - 1) << 16 | b) if m < 4 else (a << 16 | (b - 1))
            if int(field[px, py]) == want:
                x, y = px, py
                break
        else:
            raise AssertionError(f"no predecessor at {(x, y)}")
    return np.array(cells, np.int32)


def trace_many(fields, goals):
    """`goals` [G,3] = {field, x, y} -> packed paths [total,2] int32, offsets [G+1] int64, lengths [G] int64."""
    fields = np.asarray(fields, np.uint32)
    parts = []
    for f, x, y in np.asarray(goals).reshape(-1, 3):
        parts.append(trace(fields[f], (x, y)) if 0 <= f < fields.shape[0] else np.zeros((0, 2), np.int32))
    lengths = np.array([p.shape[0] for p in parts], np.int64)
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    paths = np.concatenate(parts).astype(np.int32) if parts else np.zeros((0, 2), np.int32)
    return paths.reshape(-1, 2), offsets, lengths


def make_up(cells):
    """(a, b) of a list of cells: straight and diagonal steps; asserts every step goes to an 8-neighbour."""
    d = np.abs(np.diff(np.asarray(cells, np.int64).reshape(-1, 2), axis=0))
    assert d.size == 0 or (d.max() == 1 and (d.sum(axis=1) >= 1).all())
    return int((d.sum(axis=1) == 1).sum()), int((d.sum(axis=1) == 2).sum())


# ------------------------------------------------------------------ maps
def seeded_map(shape, seed, p=0.3):
    return (np.random.default_rng(seed).random(shape) < p).astype(np.int32)


def rooms_map(n=98, room=14, doors=True):
    """Walls every `room` cells in both directions, a door in the middle of every wall segment; the room in the corner (0, 0) has no door:
    a free pocket closed by a 4-connected wall."""
    m = np.zeros((n, n), np.int32)
    for w in range(room, n, room):
        m[w, :] = 1
        m[:, w] = 1
    if doors:
        for w in range(room, n, room):
            for c in range(room // 2, n, room):
                if c % room:
                    m[w, c] = 0
                    m[c, w] = 0
    m[room, :room + 1] = 1                                       # the closed pocket
    m[:room + 1, room] = 1
    return m


def serpentine(n):
    """Walls on every odd row, each open at one end, the ends alternating: the longest way an n x n map can ask for."""
    m = np.zeros((n, n), np.int32)
    for k, x in enumerate(range(1, n, 2)):
        m[x, :] = 1
        m[x, n - 1 if k % 2 == 0 else 0] = 0
    return m
