"""The scene sensor on the device (csrc/sensor.hip; include/mi355nerf.h "scene sensor"): what the reference takes from habitat_sim
(simulator/sim.py:169-196), for a ground-truth world that is a labelled, coloured voxel grid.

`VoxelScene` is the world: uint32 words [X,Y,Z] on the device (r, g, b and the class byte, 0xFF = free) with its brick mask, built from
the procedural rooms (`from_occupancy`), a labelled point cloud (`from_point_cloud`) or a `SurfaceMesh` (`from_mesh`).  `VoxelSim` renders
it: `sample_images_from_poses(poses)` is `HabitatSim.sample_images_from_poses`, uint8 RGBA, float32 planar depth and class ids, one launch
for the whole batch, the images left on the device unless `host=True`; `cast_rays` walks given rays.

The builders are host code (numpy / torch): a scene is built once.  The walk, the rays and the shading are the header's, byte for byte."""
import ctypes
import math

import numpy as np
import torch

from . import _lib as L
from . import render as RD

FREE = 0xFF
FREE_WORD = 0xFF000000
DEPTH_PLANAR, DEPTH_RAY = 0, 1
# one byte per face: x-, x+, y- (seen from below), y+ (seen from above), z-, z+, and the near plane (the camera is inside the voxel)
DEFAULT_SHADE = (200, 200, 255, 150, 225, 225, 255)
DEFAULT_BACKGROUND = 0xFF000000                                                        # opaque black
MAX_MASK_WORDS = 16384


def _words(r, g, b, cls):
    return (np.asarray(r, np.uint32) | (np.asarray(g, np.uint32) << np.uint32(8)) | (np.asarray(b, np.uint32) << np.uint32(16))
            | (np.asarray(cls, np.uint32) << np.uint32(24))).astype(np.uint32)


def fract_bytes(n, lo, s):
    """uint8 [n]: fract of the voxel centres lo + (i + 0.5) s along one axis, quantised: min(floor(256 fract), 255)."""
    c = np.float64(lo) + (np.arange(n, dtype=np.float64) + 0.5) * np.float64(s)
    return np.minimum(np.floor((c - np.floor(c)) * 256.0), 255.0).astype(np.uint8)


def cell_classes(shape, num_classes=29):
    """int64 [X,Y,Z]: the stand-in's class of every cell, ((x 73856093) ^ (y 19349663) ^ (z 83492791)) % num_classes (standin.py:56-57)."""
    x, y, z = (np.arange(n, dtype=np.int64) for n in shape)
    return ((x[:, None, None] * 73856093) ^ (y[None, :, None] * 19349663) ^ (z[None, None, :] * 83492791)) % int(num_classes)


def occupancy_words(occ, aabb, cell=0.2, refine=4, num_classes=29, closed=False):
    """The host half of `VoxelScene.from_occupancy` -> (uint32 [X r, Y r, Z r], lo float64 [3], voxel size float64)."""
    occ = np.asarray(occ.detach().cpu().numpy() if torch.is_tensor(occ) else occ)
    occ = (occ[0] if occ.ndim == 4 else occ) != 0
    if occ.ndim != 3:
        raise ValueError(f"occ is [X,Y,Z] or [1,X,Y,Z] (got {occ.shape})")
    refine = int(refine)
    if refine < 1 or not 1 <= int(num_classes) <= FREE:
        raise ValueError("refine >= 1 and 1 <= num_classes <= 255")
    if closed:
        occ = occ.copy()
        occ[0], occ[-1], occ[:, 0], occ[:, -1], occ[:, :, 0], occ[:, :, -1] = True, True, True, True, True, True
    lo = np.asarray(aabb, np.float64).reshape(-1)[:3].copy()
    s = np.float64(cell) / np.float64(refine)
    cls = cell_classes(occ.shape, num_classes)
    fine = lambda a: np.repeat(np.repeat(np.repeat(a, refine, 0), refine, 1), refine, 2)
    X, Y, Z = (n * refine for n in occ.shape)
    r, g, b = (fract_bytes(n, lo[k], s) for k, n in enumerate((X, Y, Z)))
    colour = _words(r[:, None, None], g[None, :, None], b[None, None, :], 0)
    words = np.where(fine(occ), colour | (fine(cls).astype(np.uint32) << np.uint32(24)), np.uint32(FREE_WORD)).astype(np.uint32)
    return words, lo, float(s)


def point_cloud_words(points, colours, labels, voxel_size, lo=None):
    """The host half of `VoxelScene.from_point_cloud`: voxel floor((p - lo) / voxel_size) in float64 takes the colour and label of the LOWEST
    point index that falls into it.  `lo=None` is the cloud's least corner.  -> (uint32 [X,Y,Z], lo, voxel size)."""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    if p.shape[0] == 0 or not np.isfinite(p).all():
        raise ValueError("the cloud is empty or holds a point that is not finite")
    s = np.float64(voxel_size)
    if not s > 0:
        raise ValueError(f"voxel_size must be positive (got {voxel_size})")
    lo = p.min(axis=0) if lo is None else np.asarray(lo, np.float64).reshape(3)
    c = np.floor((p - lo) / s).astype(np.int64)
    if (c < 0).any():
        raise ValueError("a point lies below lo")
    shape = tuple(int(v) + 1 for v in c.max(axis=0))
    lin = (c[:, 0] * shape[1] + c[:, 1]) * shape[2] + c[:, 2]
    cells, first = np.unique(lin, return_index=True)                                    # the first occurrence of each: the lowest index
    col = np.full((p.shape[0], 3), 128, np.uint8) if colours is None else np.asarray(colours).reshape(-1, 3)
    lab = np.zeros(p.shape[0], np.int64) if labels is None else np.asarray(labels).reshape(-1).astype(np.int64)
    if lab.min() < 0 or lab.max() >= FREE:
        raise ValueError("labels must be in [0, 254]: 255 is the free voxel")
    words = np.full(int(np.prod(shape)), FREE_WORD, np.uint32)
    words[cells] = _words(col[first, 0], col[first, 1], col[first, 2], lab[first])
    return words.reshape(shape), lo, float(s)


class VoxelScene:
    """`voxels` uint32 words [X,Y,Z] (a numpy array, or a device tensor of int32 holding the same bits), `lo` the world position of the
    grid's corner, `voxel_size` the edge.  Lives on the device; the brick mask is built on construction (`rebuild()` after an edit)."""

    def __init__(self, voxels, lo, voxel_size, device="cuda:0"):
        if torch.is_tensor(voxels):
            v = voxels if voxels.dtype == torch.int32 else voxels.view(torch.int32)
            v = v.contiguous() if v.is_cuda else v.contiguous().to(device)
        else:
            h = np.ascontiguousarray(np.asarray(voxels, np.uint32))
            v = torch.from_numpy(h.view(np.int32)).to(device)
        if v.dim() != 3:
            raise ValueError(f"voxels is [X,Y,Z] (got {tuple(v.shape)})")
        L.require_gpu(v)
        self.voxels, self.device = v, v.device
        self.shape = tuple(int(n) for n in v.shape)
        self.lo = np.asarray(lo, np.float64).reshape(3).copy()
        self.voxel_size = float(voxel_size)
        if not (np.isfinite(self.lo).all() and math.isfinite(self.voxel_size) and self.voxel_size > 0):
            raise ValueError("lo must be finite and voxel_size positive and finite")
        self._lo_c = (ctypes.c_double * 3)(*[float(x) for x in self.lo])
        words = int(L.load_library().mnf_sensor_bricks_words(*self.shape))
        if words < 0:
            raise L.MnfError(f"a scene of {self.shape} voxels is outside the sensor's limits: a bit grid's, and a brick mask of at most {MAX_MASK_WORDS} words")
        self.bricks = torch.empty(words, dtype=torch.int32, device=self.device)
        self.rebuild()

    def rebuild(self):
        L.launch(L.load_library().mnf_sensor_build_bricks, L.ptr(self.voxels), *self.shape, L.ptr(self.bricks))

    @property
    def aabb(self):
        return np.concatenate([self.lo, self.lo + np.asarray(self.shape, np.float64) * self.voxel_size])

    def args(self):
        return (L.ptr(self.voxels), *self.shape, L.ptr(self.bricks), self._lo_c, self.voxel_size)

    @classmethod
    def from_occupancy(cls, occ, aabb, cell=0.2, refine=4, num_classes=29, closed=False, device="cuda:0"):
        """The procedural rooms (`synthetic.make_occupancy`) at `refine` voxels per cell edge: the colour of a voxel is fract of its
        centre, quantised to bytes, its class the stand-in's hash of its 0.2 m cell; `closed=True` closes the six outer faces."""
        return cls(*occupancy_words(occ, aabb, cell, refine, num_classes, closed), device=device)

    @classmethod
    def from_point_cloud(cls, points, colours, labels, voxel_size, lo=None, device="cuda:0"):
        """A semantic ground-truth cloud (`cloud.load_point_cloud_ply`): the lowest point index wins a voxel."""
        host = lambda a: None if a is None else (a.detach().cpu().numpy() if torch.is_tensor(a) else a)
        return cls(*point_cloud_words(host(points), host(colours), host(labels), voxel_size, lo), device=device)

    @classmethod
    def from_mesh(cls, mesh, voxel_size, device=None):
        """A `SurfaceMesh`, sampled by `cloud.sample_mesh_points` at half a voxel: a point takes the colour and label of its triangle's
        first vertex (grey and class 0 where the mesh has none; a label of -1 becomes 0)."""
        from . import cloud
        pts, face = cloud.sample_mesh_points(mesh, resolution=float(voxel_size) / 2)
        v0 = mesh.triangles.reshape(-1, 3)[face.long(), 0].long()
        col = None if mesh.colour is None else mesh.colour[v0]
        lab = None if mesh.label is None else mesh.label[v0].clamp(min=0)
        return cls.from_point_cloud(pts, col, lab, voxel_size, device=device or pts.device)


class VoxelSim:
    """`HabitatSim` for a `VoxelScene`: images of `img_w` x `img_h` pixels; `focal` defaults to the dataset's 0.5 W / tan(pi / 4) as
    `Dataset.update_data` evaluates it.  `info` (int64 [2] on the device) counts {misses, rays not finite} since `clear_info()`."""

    def __init__(self, scene, img_w, img_h, focal=None, near=0.0, far=1e3, shade=DEFAULT_SHADE, background=DEFAULT_BACKGROUND, device=None):
        self.scene = scene
        self.device = scene.device if device is None else torch.device(device)
        if self.device != scene.device:
            raise ValueError(f"the scene lives on {scene.device}, not on {self.device}")
        self.img_w, self.img_h = int(img_w), int(img_h)
        self.focal = float(0.5 * self.img_w / np.tan(np.pi / 2 / 2)) if focal is None else float(focal)
        self.near, self.far = float(near), float(far)
        if len(shade) != 7:
            raise ValueError("shade holds seven bytes: the six faces and the near plane")
        self._shade = (ctypes.c_uint8 * 7)(*[int(k) for k in shade])
        self.background = int(background) & 0xFFFFFFFF
        self.info = torch.zeros(2, dtype=torch.int64, device=self.device)

    def clear_info(self):
        self.info.zero_()

    @torch.no_grad()
    def render_c2w(self, c2w, depth="z", hit=False):
        """`c2w` [V,3,4] or [V,4,4] float64 (host or device) -> dict of device tensors rgba uint8 [V,H,W,4], depth float32 [V,H,W], sem uint8
        [V,H,W] and, with hit=True, hit int32 [V,H,W] (the voxel's lin or -1).  One launch; nothing is copied back."""
        if depth not in ("z", "ray"):
            raise ValueError('depth is "z" (planar, Habitat\'s) or "ray"')
        m = c2w if torch.is_tensor(c2w) else torch.from_numpy(np.ascontiguousarray(np.asarray(c2w, np.float64)))
        m = L.contig(m.to(self.device).reshape(-1, m.shape[-2], 4)[:, :3, :], torch.float64)
        V, H, W = int(m.shape[0]), self.img_h, self.img_w
        out = {"rgba": torch.empty(V, H, W, 4, dtype=torch.uint8, device=self.device), "depth": torch.empty(V, H, W, dtype=torch.float32, device=self.device),
               "sem": torch.empty(V, H, W, dtype=torch.uint8, device=self.device)}
        if hit:
            out["hit"] = torch.empty(V, H, W, dtype=torch.int32, device=self.device)
        if V:
            L.launch(L.load_library().mnf_sensor_views, *self.scene.args(), L.ptr(m), V, W, H, self.focal, self.near, self.far,
                     DEPTH_PLANAR if depth == "z" else DEPTH_RAY, self._shade, self.background, L.ptr(out["rgba"]), L.ptr(out["depth"]), L.ptr(out["sem"]),
                     L.ptr(out.get("hit")), L.ptr(self.info))
        return out

    def sample_images_from_poses(self, poses, *, host=False, depth="z", hit=False):
        """simulator/sim.py:169-196: `poses` [N,7] xyz + quaternion (x, y, z, w) -> (rgba [N,H,W,4] uint8, depth [N,H,W] float32, sem
        [N,H,W]).  The poses go through `render.pose_to_c2w` in float64.  Device tensors (sem uint8) by default; `host=True` returns numpy
        arrays shaped as Habitat's (uint8 RGBA, float32 depth, class ids widened to int64, what the dataset stores), so the reference's
        `sampled_images[:, :, :, :3]` works unchanged.  `hit=True` appends the hit voxels."""
        p = np.asarray(poses.detach().cpu().numpy() if torch.is_tensor(poses) else poses, np.float64).reshape(-1, 7)
        c2w = np.stack([RD.pose_to_c2w(q) for q in p])[:, :3, :] if p.shape[0] else np.zeros((0, 3, 4))
        out = self.render_c2w(c2w, depth=depth, hit=hit)
        res = (out["rgba"], out["depth"], out["sem"]) + ((out["hit"],) if hit else ())
        if host:
            res = tuple(t.cpu().numpy() for t in res)
            res = (res[0], res[1], res[2].astype(np.int64)) + res[3:]
        return res

    @torch.no_grad()
    def cast_rays(self, origins, dirs, near=None, far=None):
        """The walk for given rays: origins, dirs [n,3] (float64 on the device without a copy) -> dict of device tensors t_hit float64 [n]
        (-1 on a miss; in units of |dir|), hit int32 [n] (the voxel's lin or -1), face uint8 [n] (255 on a miss)."""
        f64 = lambda a: L.contig((a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64)))).to(self.device).reshape(-1, 3),
                                 torch.float64)
        o, d = f64(origins), f64(dirs)
        n = int(o.shape[0])
        if int(d.shape[0]) != n:
            raise ValueError(f"{n} origins and {int(d.shape[0])} directions")
        out = {"t_hit": torch.empty(n, dtype=torch.float64, device=self.device), "hit": torch.empty(n, dtype=torch.int32, device=self.device),
               "face": torch.empty(n, dtype=torch.uint8, device=self.device)}
        if n:
            L.launch(L.load_library().mnf_sensor_cast_rays, *self.scene.args(), L.ptr(o), L.ptr(d), n, self.near if near is None else float(near),
                     self.far if far is None else float(far), L.ptr(out["t_hit"]), L.ptr(out["hit"]), L.ptr(out["face"]), L.ptr(self.info))
        return out
