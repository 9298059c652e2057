"""What the voxel bit maps share (objects.SemanticObjectMap, explore.ExplorationMap; csrc/map_dev.h has the grid's layout): the geometry of
a grid over an aabb, the device words, and the preparation of rays and depths for an insert from tensors, rendered poses or a Dataset."""
import ctypes

import numpy as np
import torch

from . import _lib as L
from . import render as RD


def grid_resolution(aabb, voxel_size):
    """Voxels per axis that cover `aabb` = (x0, y0, z0, x1, y1, z1) at `voxel_size`: ceil of the float64 quotient (a box that is a
    whole number of voxels up to 1e-9 of a voxel gets exactly that many)."""
    a = np.asarray(aabb, np.float64).reshape(6)
    n = np.ceil((a[3:] - a[:3]) / float(voxel_size) - 1e-9).astype(np.int64)
    if (n < 1).any():
        raise ValueError(f"aabb {a.tolist()} is empty along an axis")
    return tuple(int(v) for v in n)


def planar_to_ray_scale(width, height, focal, device):
    """|cam| per pixel, row-major [H*W] float32 on `device`: the factor that turns a planar (z) depth into the length along the pixel's
    normalised ray, cam = ((x - W/2 + 0.5) / f, (y - H/2 + 0.5) / f, 1)."""
    f = float(np.float32(focal))
    x = (torch.arange(width, device=device, dtype=torch.float32) - width / 2 + 0.5) / f
    y = (torch.arange(height, device=device, dtype=torch.float32) - height / 2 + 0.5) / f
    return torch.sqrt(x[None, :] * x[None, :] + y[:, None] * y[:, None] + 1.0).reshape(-1)


class VoxelBitMap:
    """A persistent bit grid uint32 [planes, words] over the voxels of `aabb`.  `map_bytes(resolution)` is the library's byte function
    for the grid (0: more than the map indexes); `what` names the grid in that error."""

    def __init__(self, aabb, voxel_size, planes, map_bytes, device, what=""):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise L.MnfError(f"{type(self).__name__} lives on a GPU; there is no CPU fallback")
        self.voxel_size = float(np.float32(voxel_size))
        self.resolution = grid_resolution(aabb, voxel_size)
        self.grid_min = np.asarray(aabb, np.float64).reshape(6)[:3].astype(np.float32)
        self._gmin = (ctypes.c_float * 3)(*[float(v) for v in self.grid_min])
        nbytes = int(map_bytes(self.resolution))
        if nbytes <= 0:
            raise ValueError(f"{what}{self.resolution} voxels are more than the map indexes")
        self.words_per_plane = nbytes // (4 * planes)
        self.bits = torch.zeros(planes, self.words_per_plane, dtype=torch.int32, device=self.device)     # uint32 words

    def clear(self):
        self.bits.zero_()

    @staticmethod
    def _flat_rays(rays_o, rays_d, depth, acc):
        """-> (origins [n,3], directions [n,3], depth [n], acc [n] or None, n): contiguous float32."""
        o, d = L.contig(rays_o.reshape(-1, 3), torch.float32), L.contig(rays_d.reshape(-1, 3), torch.float32)
        dep = L.contig(depth.reshape(-1), torch.float32)
        n = int(dep.shape[0])
        if int(o.shape[0]) != n or int(d.shape[0]) != n:
            raise ValueError(f"{int(o.shape[0])} origins and {int(d.shape[0])} directions for {n} depths")
        a = None
        if acc is not None:
            a = L.contig(acc.reshape(-1), torch.float32)
            if int(a.shape[0]) != n:
                raise ValueError(f"{int(a.shape[0])} acc values for {n} depths")
        return o, d, dep, a, n

    def _render_poses(self, radiance_field, estimator, poses, width, height, focal, near_plane, render_step_size, scale, cone_angle, alpha_thre):
        """`poses` rendered exactly as `render_image_from_pose` renders them (the same rays, the same `render_views` call, background
        zeros) -> (origins, directions, the render's dict of device tensors)."""
        o, d, h, w = RD._pose_rays(np.asarray(poses), width, height, focal, scale, self.device)
        r = RD.render_views(radiance_field, estimator, o, d, h * w, 1024, near_plane=near_plane, render_step_size=render_step_size,
                            render_bkgd=torch.zeros(3), cone_angle=cone_angle, alpha_thre=alpha_thre, image_hw=(h, w), n_split=None)
        return o, d, r

    def _dataset_rays(self, dataset, image_ids, depth_along):
        """Views `image_ids` of a `Dataset`, either storage layout -> (ids, rays from `generate_image_rays` on the dataset's poses and
        K, the stored depth as ray length [V, H*W] float32), or None for no view.  `depth_along="z"`: the stored depth is Habitat's
        planar depth and the ray length is z * |cam| (planar_to_ray_scale); `"ray"`: the stored depth is the ray length."""
        if depth_along not in ("z", "ray"):
            raise ValueError('depth_along is "z" or "ray"')
        ids = RD._eval_index_tensor(image_ids, self.device, len(dataset), "image_ids")
        if int(ids.shape[0]) == 0:
            return None
        L.require_gpu(dataset.depths, dataset.camtoworlds)
        H, W = int(dataset.height), int(dataset.width)
        rays = RD.generate_image_rays(dataset.camtoworlds[ids], W, H, dataset.K, self.device)
        depth = dataset.depths[ids].reshape(-1, H * W).to(torch.float32)
        if depth_along == "z":
            depth = depth * planar_to_ray_scale(W, H, float(dataset.K[0, 0]), self.device)[None]
        return ids, rays, depth
