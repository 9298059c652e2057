"""TSDF fusion of captures on the device (csrc/tsdf.hip; include/mi355nerf.h "TSDF fusion of captures"): the truncated signed distance
volume a classical robotics stack builds from the depth, colour and class images the field is trained on, so that the neural map can be
judged beside it: `vol.integrate_dataset(ds, ids); vol.extract_mesh().quality(gt)` next to `extract_surface(field, est, iso).quality(gt)`.

Nearest-pixel lookup without interpolation; one truncation for the whole volume; a point's colour and class are those of the observation
closest to the surface, not an average; the mesh is open where nothing was observed.  Fusing rendered views of the field is not part of
this.  Only `info`, `counts` and a mesh the caller asks for on the host cross the bus."""
import ctypes

import numpy as np
import torch

from . import _lib as L
from . import surface as SF
from .voxelmap import grid_resolution

DEPTH_MODES = {"z": 0, "ray": 1}
INFO_KEYS = ("applied", "first_observed", "invalid_depth", "behind_surface", "label_out_of_range")
MAX_VIEWS = 65535


class TsdfVolume:
    """Lattice points [X+1, Y+1, Z+1] over `aabb` at `voxel_size` metres (X, Y, Z from `voxelmap.grid_resolution`, 1 .. 1024 each): `tsdf`
    float32 (1 where nothing was seen), `weight` int32 (observations, capped at `max_weight`), `word` int32 holding the sensor's uint32
    voxel word (r, g, b, class) and `best` float32 (the |sdf| of the observation that wrote the word, -1 for none).  `trunc=None` is 4
    voxels.  Lives on a GPU; there is no CPU fallback."""

    def __init__(self, aabb, voxel_size, trunc=None, max_weight=64, max_depth=10.0, min_depth=0.0, device="cuda:0"):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise L.MnfError("TsdfVolume lives on a GPU; there is no CPU fallback")
        self.voxel_size = float(voxel_size)
        self.cells = grid_resolution(aabb, voxel_size)
        if max(self.cells) > 1024:
            raise ValueError(f"{self.cells} cells are more than the 1024 per axis the lattice holds")
        self.lo = np.asarray(aabb, np.float64).reshape(6)[:3].copy()
        self._lo_c = (ctypes.c_double * 3)(*[float(v) for v in self.lo])
        self.trunc = 4.0 * self.voxel_size if trunc is None else float(trunc)
        self.max_weight, self.max_depth, self.min_depth = int(max_weight), float(max_depth), float(min_depth)
        self.shape = tuple(c + 1 for c in self.cells)
        dev = self.device
        self.tsdf = torch.empty(self.shape, dtype=torch.float32, device=dev)
        self.weight = torch.empty(self.shape, dtype=torch.int32, device=dev)
        self.word = torch.empty(self.shape, dtype=torch.int32, device=dev)
        self.best = torch.empty(self.shape, dtype=torch.float32, device=dev)
        self.info_device = torch.empty(5, dtype=torch.int64, device=dev)
        self.clear()

    def clear(self):
        self.tsdf.fill_(1.0)
        self.weight.zero_()
        self.word.zero_()
        self.best.fill_(-1.0)
        self.info_device.zero_()

    @property
    def aabb(self):
        return np.concatenate([self.lo, self.lo + np.asarray(self.cells, np.float64) * self.voxel_size])

    # ------------------------------------------------------------------ fusion
    def _call(self, depth, colour, classes, c2w, focal, mode):
        V, H, W = (int(n) for n in depth.shape)
        if V > MAX_VIEWS:
            raise ValueError(f"{V} views in one call (at most {MAX_VIEWS})")
        L.launch(L.load_library().mnf_tsdf_integrate, L.ptr(self.tsdf), L.ptr(self.weight), L.ptr(self.word), L.ptr(self.best), *self.cells, self._lo_c,
                 self.voxel_size, self.trunc, self.max_weight, self.min_depth, self.max_depth, L.ptr(c2w), V, W, H, float(focal), L.ptr(depth),
                 1 if depth.dtype == torch.float16 else 0, L.ptr(colour), int(colour.shape[-1]), L.ptr(classes), 1 if classes.dtype == torch.int64 else 0, mode,
                 L.ptr(self.info_device))

    def _checked(self, depth, colour, classes, c2w):
        if depth.dim() == 4 and depth.shape[-1] == 1:
            depth = depth[..., 0]
        if depth.dim() != 3 or depth.dtype not in (torch.float32, torch.float16):
            raise ValueError(f"depth is [V,H,W] float32 or float16 (got {tuple(depth.shape)} {depth.dtype})")
        V, H, W = depth.shape
        if colour.dtype != torch.uint8 or tuple(colour.shape[:3]) != (V, H, W) or colour.dim() != 4 or colour.shape[-1] not in (3, 4):
            raise ValueError(f"colour is uint8 [V,H,W,3] or [V,H,W,4] (got {tuple(colour.shape)} {colour.dtype})")
        if classes.dtype not in (torch.uint8, torch.int64) or tuple(classes.shape) != (V, H, W):
            raise ValueError(f"classes is uint8 or int64 [V,H,W] (got {tuple(classes.shape)} {classes.dtype})")
        if c2w.dim() != 3 or int(c2w.shape[0]) != V or c2w.shape[-1] != 4 or c2w.shape[-2] not in (3, 4):
            raise ValueError(f"c2w is [V,3,4] or [V,4,4] (got {tuple(c2w.shape)})")
        return depth.contiguous(), colour.contiguous(), classes.contiguous(), L.contig(c2w[:, :3, :], torch.float64)

    def _up(self, a, dtype=None):
        t = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype)))
        return t.to(self.device)

    @torch.no_grad()
    def integrate(self, depth, colour, classes, c2w, focal, depth_along="z"):
        """Fuse V captures, in order: depth [V,H,W] float32 or float16, colour uint8 [V,H,W,3] or the sensor's RGBA [V,H,W,4] unsliced,
        classes uint8 or int64 [V,H,W], c2w [V,3,4] or [V,4,4] (widened to float64), `focal` in pixels.  Device tensors straight from
        `VoxelSim.sample_images_from_poses` are used as they are; host arrays go up once.  `depth_along` is "z" (planar depth, Habitat's)
        or "ray" (the length of the pixel's ray).  One launch, no synchronisation."""
        if depth_along not in DEPTH_MODES:
            raise ValueError('depth_along is "z" or "ray"')
        d, c, k, m = self._checked(self._up(depth), self._up(colour), self._up(classes), self._up(c2w, np.float64))
        if int(d.shape[0]):
            self._call(d, c, k, m, focal, DEPTH_MODES[depth_along])

    @torch.no_grad()
    def integrate_dataset(self, dataset, image_ids, depth_along="z"):
        """Fuse views `image_ids` of a `Dataset`, in that order, either storage layout (uint8 / float32 / int64 or uint8 / float16 /
        uint8), with the dataset's poses and focal.  No image is copied: every run of consecutive ids is one launch on the dataset's own
        storage, and V views in one call give the bytes of V calls."""
        if depth_along not in DEPTH_MODES:
            raise ValueError('depth_along is "z" or "ray"')
        ids = np.asarray(image_ids.cpu() if torch.is_tensor(image_ids) else image_ids).astype(np.int64).reshape(-1)
        if ids.size == 0:
            return
        if ids.min() < 0 or ids.max() >= len(dataset):
            raise IndexError(f"image_ids out of range [0, {len(dataset)})")
        L.require_gpu(dataset.images, dataset.depths, dataset.semantics, dataset.camtoworlds)
        focal = float(dataset.K[0, 0])
        start = 0
        for i in range(1, ids.size + 1):
            if i == ids.size or ids[i] != ids[i - 1] + 1 or i - start == MAX_VIEWS:
                a, b = int(ids[start]), int(ids[i - 1]) + 1
                d, c, k, m = self._checked(dataset.depths[a:b], dataset.images[a:b], dataset.semantics[a:b], dataset.camtoworlds[a:b])
                self._call(d, c, k, m, focal, DEPTH_MODES[depth_along])
                start = i

    # ------------------------------------------------------------------ read-outs
    def info(self):
        """dict of the five counters since `clear()`: observations applied, points observed for the first time, invalid depths,
        observations behind the surface, labels out of range."""
        return dict(zip(INFO_KEYS, (int(v) for v in self.info_device.cpu().numpy())))

    @torch.no_grad()
    def _lattice(self, min_weight):
        values = torch.empty(self.shape, dtype=torch.float32, device=self.device)
        counts = torch.empty(3, dtype=torch.int64, device=self.device)
        L.launch(L.load_library().mnf_tsdf_lattice, L.ptr(self.tsdf), L.ptr(self.weight), L.ptr(self.best), *self.cells, int(min_weight), L.ptr(values),
                 L.ptr(counts))
        return values, counts

    def lattice(self, min_weight=1):
        """float32 device tensor [X+1, Y+1, Z+1]: -tsdf where weight >= min_weight, NaN (unobserved) elsewhere; positive is behind a surface."""
        return self._lattice(min_weight)[0]

    def counts(self, min_weight=1):
        """dict(observed, inside, worded, points, observed_fraction)."""
        obs, inside, worded = (int(v) for v in self._lattice(min_weight)[1].cpu().numpy())
        n = int(np.prod(self.shape))
        return {"observed": obs, "inside": inside, "worded": worded, "points": n, "observed_fraction": obs / n}

    @torch.no_grad()
    def vertex_attrs(self, positions, palette=None):
        """positions [n,3] float32 on the device -> dict(colour uint8 [n,3], label int32 [n] (-1: no observed corner), and with a `palette`
        [K,3] uint8: sem_colour uint8 [n,3])."""
        L.require_gpu(positions)
        pos = L.contig(positions.reshape(-1, 3), torch.float32)
        n = int(pos.shape[0])
        out = {"colour": torch.empty(n, 3, dtype=torch.uint8, device=self.device), "label": torch.empty(n, dtype=torch.int32, device=self.device)}
        pal = None
        if palette is not None:
            pal = palette if torch.is_tensor(palette) else torch.from_numpy(np.ascontiguousarray(palette, np.uint8))
            pal = L.contig(pal.to(self.device), torch.uint8)
            if pal.dim() != 2 or int(pal.shape[1]) != 3 or int(pal.shape[0]) < 1:
                raise ValueError(f"palette is [K, 3] (got {tuple(pal.shape)})")
            out["sem_colour"] = torch.empty(n, 3, dtype=torch.uint8, device=self.device)
        if n:
            L.launch(L.load_library().mnf_tsdf_vertex_attrs, L.ptr(self.word), L.ptr(self.best), *self.cells, self._lo_c, self.voxel_size, L.ptr(pos), n,
                     L.ptr(pal), 0 if pal is None else int(pal.shape[0]), L.ptr(out["colour"]), L.ptr(out["label"]), L.ptr(out.get("sem_colour")))
        return out

    @torch.no_grad()
    def extract_mesh(self, min_weight=1, palette=None, max_vertices=None, max_triangles=None):
        """The fused surface: the zero set of the lattice by the observed-only extractor (`mnf_surface_extract_observed`), with the
        colour, class and, with a `palette`, class colour of every vertex (`mnf_tsdf_vertex_attrs`).  -> `SurfaceMesh` on the device.
        Capacities as in `surface.extract_lattice_surface`: none given, a counting pass sizes the outputs."""
        origin = self.lo.astype(np.float32)
        step = np.full(3, np.float32(self.voxel_size), np.float32)
        mesh = SF.extract_lattice_surface(self.lattice(min_weight), 0.0, origin, step, max_vertices, max_triangles, observed=True)
        a = self.vertex_attrs(mesh.positions, palette)
        mesh.colour, mesh.label, mesh.sem_colour = a["colour"], a["label"], a.get("sem_colour")
        return mesh
