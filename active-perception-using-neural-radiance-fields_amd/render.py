"""Render orchestration with the reference's names and signatures
(perception/models/utils.py, perception/data_proc/habitat_to_data.py, scripts/pipeline.py:666-798),
running on libmi355nerf.so.

  Rays                                            perception/models/datasets/utils.py:7
  render_image_with_occgrid_test                  utils.py:555-779
  render_probablistic_image_with_occgrid_test     utils.py:782-1032
  render_image_with_occgrid_with_depth_guide      utils.py:63-219   (forward; see DESIGN.md §Scope for backward)
  fused_train_render                              utils.py:63-219 on the one-call step's kernels, differentiable (any torch loss behind it)
  fused_train_render_rays                         the same, also differentiable with respect to the rays (a pose refiner behind transform_rays)
  sem_rendering                                   utils.py:362-461
  generate_image_rays / render_*_from_pose        habitat_to_data.py:274-549
  probablistic_uncertainty -> score_views         pipeline.py:666-798
"""
import collections
import ctypes
import weakref
from typing import Optional

import numpy as np
import torch

from . import _lib as L
from . import nerfacc as NA

Rays = collections.namedtuple("Rays", ("origins", "viewdirs"))
_GridArgs = collections.namedtuple("_GridArgs", ("binaries", "bits", "occs", "res", "aabb", "n_levels"))       # `_grid_args`

_WORKSPACES = collections.OrderedDict()
MAX_CACHED_WORKSPACES = 12      # (device, slot, stream) entries kept; the least recently used one goes first.  Grows to the largest job count of a render call + 4


def _workspace(key, nbytes: int) -> torch.Tensor:
    """Cached scratch buffer; `key` is a device or (device, slot) — concurrent render jobs of one call use one slot each.  The buffer belongs to the
    (device, slot) AND the stream the caller enqueues on: two members of an ensemble trained or rendered side by side on two streams must not share
    scratch (round 4: they did, silently, through the per-device cache).
    Cost: one buffer per (device, slot, stream) in use, sized for that key's largest call so far — hundreds of MB for a train step (feature rows, bin lists).
    At most MAX_CACHED_WORKSPACES entries are kept (least recently used evicted: a caller that makes streams per phase or per epoch no longer accumulates
    buffers); `release_workspaces(stream)` drops a stream's buffers at once.  Eviction is safe while kernels still use a buffer: it was allocated
    under the stream it is keyed by, so torch's caching allocator hands its memory only to later work of that same stream."""
    device = key[0] if isinstance(key, tuple) else key
    key = (key, torch.cuda.current_stream(device).cuda_stream) if torch.device(device).type == "cuda" else key
    ws = _WORKSPACES.get(key)
    if ws is None or ws.numel() < nbytes:
        _WORKSPACES[key] = ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
    _WORKSPACES.move_to_end(key)
    while len(_WORKSPACES) > MAX_CACHED_WORKSPACES:
        _WORKSPACES.popitem(last=False)
    return ws


def release_workspaces(stream=None):
    """Drop the cached workspaces: all of them, or those keyed by `stream` (a torch.cuda.Stream or a raw handle)."""
    if stream is None:
        _WORKSPACES.clear()
        return
    h = getattr(stream, "cuda_stream", stream)
    for k in [k for k in _WORKSPACES if isinstance(k, tuple) and len(k) == 2 and k[1] == h]:
        del _WORKSPACES[k]


def _grid_args(estimator, max_levels=4):
    """The occupancy grid as the C entry points take it: the binaries as u8 [L,X,Y,Z], the estimator's packed bit grid (no per-call packing), its
    occupancy values, the resolution (X, Y, Z) and the L aabbs as one `c_float` array of 6 L.  The host copy of the aabbs lives on the estimator
    and is refreshed when the tensor changes (`OccGridEstimator.aabb_host`), so a call does not synchronise."""
    L_ = int(estimator.binaries.shape[0])
    if L_ > max_levels:
        raise NotImplementedError(f"the fused renderer supports up to {max_levels} occupancy levels (got {L_}); use nerfacc.traverse_grids")
    b = estimator.binaries
    b = b.contiguous().view(torch.uint8) if b.dtype == torch.bool else b.to(torch.uint8).contiguous()
    L.require_gpu(b)
    aabb = [x for lvl in range(L_) for x in estimator.aabb_host(lvl)]
    bits = estimator.bitgrid() if hasattr(estimator, "bitgrid") else None
    return _GridArgs(b, bits, estimator.occs, tuple(b.shape[1:]), (ctypes.c_float * len(aabb))(*aabb), L_)


def _render_opts(*, max_samples, near_plane, far_plane, render_step_size, cone_angle, alpha_thre, early_stop_eps, probabilistic, rays_per_view,
                 sync_every=8, render_bkgd=None, view_order=None, n_levels=0):
    """`mnf_render_opts` (include/mi355nerf.h).  `render_bkgd`: read on the host (None: black); `view_order`: `_view_order`'s (None: row-major)."""
    opts = L.RenderOpts()
    opts.near_plane, opts.far_plane, opts.render_step_size = near_plane, far_plane, render_step_size
    opts.cone_angle, opts.alpha_thre, opts.early_stop_eps = cone_angle, alpha_thre, early_stop_eps
    for i, x in enumerate(() if render_bkgd is None else render_bkgd.detach().cpu().reshape(-1)[:3]):
        opts.render_bkgd[i] = float(x)
    opts.max_samples, opts.probabilistic, opts.rays_per_view, opts.sync_every = int(max_samples), int(probabilistic), int(rays_per_view), sync_every
    opts.view_order, opts.bitgrid, opts.n_levels = (None if view_order is None else view_order.data_ptr()), None, n_levels
    return opts


_VIEW_ORDERS = {}


def _view_order(h: int, w: int, device, block: int = 8) -> torch.Tensor:
    """Device int32 permutation of the h*w row-major pixels of a view into block x block tiles (tiles row-major, pixels
    row-major inside a tile): the order in which the renderer marches a view's rays (`mnf_render_opts.view_order`).
    A 64-sample tile of the field kernel then covers a compact pixel patch instead of a one-pixel-high strip and touches
    fewer hash-table lines (-5 % render time at 800x800); results are per ray and do not depend on it."""
    key = (h, w, block, str(device))
    t = _VIEW_ORDERS.get(key)
    if t is None:
        ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
        k = ((ys // block) * ((w + block - 1) // block) + xs // block) * (block * block) + (ys % block) * block + xs % block
        t = torch.from_numpy(np.argsort(k.reshape(-1), kind="stable").astype(np.int32)).to(device)
        _VIEW_ORDERS[key] = t
    return t


def _render_jobs(specs, rpv, *, max_samples, near_plane, far_plane, render_step_size, render_bkgd, cone_angle, alpha_thre, early_stop_eps,
                 probabilistic, sync_every=8, image_hw=None, n_split=2):
    """`specs`: list of (radiance_field, estimator, origins [n,3], viewdirs [n,3]) sharing rays_per_view `rpv` and every option (the
    members of an ensemble looking at the same poses, or one model).  Every spec is cut into up to `n_split` contiguous groups of
    whole views, and all (spec, group) pairs advance side by side as render jobs of ONE C call (`mnf_render_jobs`): while one job's
    marcher or the tail of its field launch leaves compute units idle, the other jobs' kernels use them.  A view's result does not
    depend on the grouping (its round schedule and its sample tiles are its own).  Returns one dict of device tensors per spec."""
    lib = L.load_library()
    dev = specs[0][2].device                         # the GPU that owns the rays: device guard + stream of the call
    order = _view_order(*image_hw, dev) if image_hw is not None and image_hw[0] * image_hw[1] == rpv and min(image_hw) >= 16 else None
    opts = _render_opts(max_samples=max_samples, near_plane=near_plane, far_plane=far_plane, render_step_size=render_step_size, cone_angle=cone_angle,
                        alpha_thre=alpha_thre, early_stop_eps=early_stop_eps, probabilistic=probabilistic, rays_per_view=rpv, sync_every=sync_every,
                        render_bkgd=render_bkgd, view_order=order)
    # n_split=None: the measured optimum for the shape — small views (the scorer's 64 x 64 sub-samples: a round is latency-bound) advance as four jobs, full
    # images as two (profiles/r03_hw_queues.txt: one member, 256 scoring views 54.3 -> 50.4 ms with four; 800 x 800 views: two and four tie)
    want = (4 if rpv <= 16384 else 2) if n_split is None else int(n_split)
    groups = [max(1, min(want, o.shape[0] // rpv)) for _, _, o, _ in specs]
    global MAX_CACHED_WORKSPACES
    MAX_CACHED_WORKSPACES = max(MAX_CACHED_WORKSPACES, sum(groups) + 4)      # a call never evicts the slots it is still filling: the cap follows the largest job count seen
    jobs, keep, outs, grid0 = [], [], [], None
    for (radiance_field, estimator, o, d), G in zip(specs, groups):
        L.require_gpu(o, d)
        n, C = o.shape[0], radiance_field.num_semantic_classes
        if n % rpv:
            raise L.MnfError(f"n_rays ({n}) must be a positive multiple of rays_per_view ({rpv})")
        handle, grid = radiance_field._ensure_handle(), _grid_args(estimator)
        if grid0 is None:
            grid0 = grid
        elif (grid0.res, tuple(grid0.aabb)) != (grid.res, tuple(grid.aabb)):
            raise L.MnfError("render jobs of one call must share the occupancy grid resolution and aabb")
        rgb = torch.empty(n, 3, device=dev); acc = torch.empty(n, 1, device=dev); depth = torch.empty(n, 1, device=dev)
        sem = torch.empty(n, C, device=dev)
        rgb_var, depth_var = (torch.empty(n, 3, device=dev), torch.empty(n, 1, device=dev)) if probabilistic else (None, None)
        V = n // rpv
        totals = torch.zeros(G, 2, dtype=torch.int64, device=dev)   # per job: [kept (reference total_samples), evaluated]
        keep += [grid, o, d, totals]
        for g in range(G):
            r0, r1 = (V * g // G) * rpv, (V * (g + 1) // G) * rpv
            if r1 == r0:
                continue
            nbytes = lib.mnf_render_workspace_bytes(r1 - r0, rpv)
            ws = _workspace((dev, len(jobs)), nbytes)
            j = L.RenderJob()
            j.field, j.binaries, j.bitgrid = handle, grid.binaries.data_ptr(), (None if grid.bits is None else grid.bits.data_ptr())
            j.rays_o, j.rays_d, j.n_rays = o[r0:].data_ptr(), d[r0:].data_ptr(), r1 - r0
            j.rgb, j.acc, j.depth, j.sem = rgb[r0:].data_ptr(), acc[r0:].data_ptr(), depth[r0:].data_ptr(), sem[r0:].data_ptr()
            j.rgb_var, j.depth_var = (rgb_var[r0:].data_ptr(), depth_var[r0:].data_ptr()) if probabilistic else (None, None)
            j.total_samples = totals[g].data_ptr()
            j.workspace, j.workspace_bytes = ws.data_ptr(), nbytes
            jobs.append(j)
            keep.append(ws)
        outs.append(dict(rgb=rgb, acc=acc, depth=depth, sem=sem, _totals=totals, **(dict(rgb_var=rgb_var, depth_var=depth_var) if probabilistic else {})))
    if jobs:
        opts.n_levels = grid0.n_levels
        L.launch(lib.mnf_render_jobs, (L.RenderJob * len(jobs))(*jobs), len(jobs), *grid0.res, grid0.aabb, ctypes.byref(opts), device=dev)
    for out in outs:
        out["total"] = out.pop("_totals").sum(0)
    return outs


def _render_test(radiance_field, estimator, rays, rays_per_view=None, image_hw=None, **jobs_kw):
    """One model's test render through `_render_jobs` (whose keywords `jobs_kw` are), reshaped to the rays' leading shape."""
    rays_shape = rays.origins.shape
    if image_hw is None and rays_per_view is None and len(rays_shape) == 3:
        image_hw = (int(rays_shape[0]), int(rays_shape[1]))      # [H,W,3] rays (utils.py:574-580): one image
    o = L.contig(rays.origins.reshape(-1, 3), torch.float32)
    d = L.contig(rays.viewdirs.reshape(-1, 3), torch.float32)
    L.require_gpu(o, d)
    n, dev = o.shape[0], o.device
    if n == 0:
        widths = dict(rgb=3, acc=1, depth=1, sem=radiance_field.num_semantic_classes, **(dict(rgb_var=3, depth_var=1) if jobs_kw["probabilistic"] else {}))
        out = dict({k: torch.empty(0, c, device=dev) for k, c in widths.items()}, total=torch.zeros(2, dtype=torch.int64, device=dev))
    else:
        out = _render_jobs([(radiance_field, estimator, o, d)], n if rays_per_view is None else int(rays_per_view), image_hw=image_hw, **jobs_kw)[0]
    return {k: v if k == "total" else v.view(*rays_shape[:-1], -1) for k, v in out.items()}


@torch.no_grad()
def render_image_with_occgrid_test(max_samples: int, radiance_field, estimator, rays: Rays, near_plane: float = 0.0,
                                   far_plane: float = 1e10, render_step_size: float = 1e-3,
                                   render_bkgd: Optional[torch.Tensor] = None, cone_angle: float = 0.0,
                                   alpha_thre: float = 0.0, early_stop_eps: float = 1e-4, timestamps=None):
    """utils.py:555-779 -> (rgb, acc, depth, sem, total_samples)."""
    if timestamps is not None:
        raise NotImplementedError("timestamps (D-NeRF) are not part of the hot path")
    r = _render_test(radiance_field, estimator, rays, max_samples=max_samples, near_plane=near_plane, far_plane=far_plane, render_step_size=render_step_size,
                     render_bkgd=render_bkgd, cone_angle=cone_angle, alpha_thre=alpha_thre, early_stop_eps=early_stop_eps, probabilistic=False)
    return r["rgb"], r["acc"], r["depth"], r["sem"], int(r["total"][0].item())


@torch.no_grad()
def render_probablistic_image_with_occgrid_test(max_samples: int, radiance_field, estimator, rays: Rays,
                                                near_plane: float = 0.0, far_plane: float = 1e10,
                                                render_step_size: float = 1e-3, render_bkgd: Optional[torch.Tensor] = None,
                                                cone_angle: float = 0.0, alpha_thre: float = 0.0,
                                                early_stop_eps: float = 1e-4, timestamps=None):
    """utils.py:782-1032 -> (rgb, rgb_var, acc, depth, depth_var, sem, total_samples)."""
    if timestamps is not None:
        raise NotImplementedError("timestamps (D-NeRF) are not part of the hot path")
    r = _render_test(radiance_field, estimator, rays, max_samples=max_samples, near_plane=near_plane, far_plane=far_plane, render_step_size=render_step_size,
                     render_bkgd=render_bkgd, cone_angle=cone_angle, alpha_thre=alpha_thre, early_stop_eps=early_stop_eps, probabilistic=True)
    return r["rgb"], r["rgb_var"], r["acc"], r["depth"], r["depth_var"], r["sem"], int(r["total"][0].item())


@torch.no_grad()
def render_views(radiance_field, estimator, rays_o, rays_d, rays_per_view, max_samples=1024, near_plane=0.0,
                 far_plane=1e10, render_step_size=1e-3, render_bkgd=None, cone_angle=0.0, alpha_thre=0.0,
                 early_stop_eps=1e-4, probabilistic=False, sync_every=8, image_hw=None, n_split=2):
    """Batched form: rays_o/rays_d [V*rays_per_view, 3]; every group of rays_per_view rays is rendered exactly as one
    call of the reference function (own round schedule).  `image_hw=(H, W)` says that the rays of a view are the row-major
    pixels of an H x W image (a speed hint only: see `_view_order`).  `n_split`: the views are rendered as up to this many
    groups advancing side by side (`_render_jobs`; a speed choice only: results do not depend on it).
    Returns a dict of device tensors."""
    return _render_test(radiance_field, estimator, Rays(rays_o, rays_d), rays_per_view, image_hw, max_samples=max_samples, near_plane=near_plane,
                        far_plane=far_plane, render_step_size=render_step_size, render_bkgd=render_bkgd, cone_angle=cone_angle, alpha_thre=alpha_thre,
                        early_stop_eps=early_stop_eps, probabilistic=probabilistic, sync_every=sync_every, n_split=n_split)


# ------------------------------------------------------------------ train-mode forward (utils.py:63-219, :362-461)
_CompositeTrain = NA._CompositeTrain     # csrc/composite_train.hip behind autograd (defined next to `rendering`)


def sem_rendering(radiance_field, rays: Rays, t_starts, t_ends, ray_indices, n_rays, render_bkgd=None):
    """utils.py:362-461 on packed samples.  With autograd enabled and a parameter — or, for a field with `forward_samples_grad`, `rays.origins` /
    `rays.viewdirs` — requiring a gradient, the field is evaluated through its differentiable forward: the closure of utils.py:122-137 inside the kernel
    (`forward_samples_grad`, which also returns the gradients of the rays), or in torch for a field without it or for distances that themselves want
    gradients; the result is composited by `_CompositeTrain`.  Otherwise the fused no-grad kernel."""
    C = radiance_field.num_semantic_classes
    dev = t_starts.device
    in_kernel = hasattr(radiance_field, "forward_samples_grad")
    differentiable = torch.is_grad_enabled() and (any(p.requires_grad for p in radiance_field.parameters())
                                                  or (in_kernel and (rays.origins.requires_grad or rays.viewdirs.requires_grad)))
    if t_starts.shape[0] != 0 and differentiable and in_kernel and not (t_starts.requires_grad or t_ends.requires_grad):
        rgbs, sigmas, sems = radiance_field.forward_samples_grad(rays.origins, rays.viewdirs, ray_indices, t_starts, t_ends)
        sigmas = sigmas.squeeze(-1)
    elif t_starts.shape[0] != 0 and differentiable:
        t_dirs = rays.viewdirs[ray_indices]
        positions = rays.origins[ray_indices] + t_dirs * (t_starts + t_ends)[:, None] / 2.0
        rgbs, sigmas, sems = radiance_field(positions, t_dirs)
        sigmas = sigmas.squeeze(-1)
    elif t_starts.shape[0] != 0:
        rgbs, sigmas, sems = radiance_field.forward_samples(rays.origins, rays.viewdirs, ray_indices, t_starts, t_ends)
    else:
        rgbs, sigmas, sems = torch.empty((0, 3), device=dev), torch.empty((0,), device=dev), torch.empty((0, C), device=dev)
    packed = NA.pack_info_grouped(ray_indices, n_rays)
    bk = None if render_bkgd is None else render_bkgd.to(device=dev, dtype=torch.float32).reshape(3).contiguous()
    colors, opacities, depths, semantics, weights, trans, alphas = _CompositeTrain.apply(
        packed[:, 0].contiguous(), packed[:, 1].contiguous(), t_starts, t_ends, sigmas, rgbs, sems, bk)
    return colors, opacities, depths, semantics, dict(weights=weights, alphas=alphas, trans=trans, sigmas=sigmas, rgbs=rgbs)


def render_image_with_occgrid_with_depth_guide(radiance_field, estimator, rays: Rays, near_plane: float = 0.0,
                                               far_plane: float = 1e10, render_step_size: float = 1e-3,
                                               render_bkgd: Optional[torch.Tensor] = None, cone_angle: float = 0.0,
                                               alpha_thre: float = 0.0, test_chunk_size: int = 8192, timestamps=None,
                                               depth: Optional[torch.Tensor] = None):
    """utils.py:63-219: occupancy sampling with the density pre-pass (no grad), then semantic volume rendering.
    Differentiable w.r.t. the field parameters when autograd is enabled (the reference's training forward);
    `depth` is accepted and ignored as in the reference."""
    if timestamps is not None:
        raise NotImplementedError("timestamps (D-NeRF) are not part of the hot path")
    rays_shape = rays.origins.shape
    o, d = rays.origins.reshape(-1, 3), rays.viewdirs.reshape(-1, 3)
    num_rays = o.shape[0]
    chunk = torch.iinfo(torch.int32).max if radiance_field.training else test_chunk_size
    results = []
    for i in range(0, num_rays, chunk):
        co, cd = o[i:i + chunk], d[i:i + chunk]

        from .ngp import RaySigmaFn
        sigma_fn = RaySigmaFn(radiance_field, co, cd)      # utils.py:89-101; lets `sampling` skip what lies behind opaque surfaces

        ray_indices, t_starts, t_ends = estimator.sampling(co, cd, sigma_fn=sigma_fn, near_plane=near_plane, far_plane=far_plane,
                                                           render_step_size=render_step_size, stratified=radiance_field.training,
                                                           cone_angle=cone_angle, alpha_thre=alpha_thre, depth=depth)
        rgb, opacity, dep, semantics, _ = sem_rendering(radiance_field, Rays(co, cd), t_starts, t_ends, ray_indices, co.shape[0],
                                                        render_bkgd)
        results.append((rgb, opacity, dep, semantics, len(t_starts)))
    colors, opacities, depths, semantics = (torch.cat([r[k] for r in results], 0) for k in range(4))
    shp = tuple(rays_shape[:-1])
    return colors.view(*shp, -1), opacities.view(*shp, -1), depths.view(*shp, -1), semantics.view(*shp, -1), sum(r[4] for r in results)


def transform_rays(rays: Rays, rotvec: torch.Tensor, trans: torch.Tensor) -> Rays:
    """Rays under the rigid motion a pose refiner optimises, as a 6-vector (rotvec [3] axis-angle, trans [3]): directions are rotated by the Rodrigues
    matrix R = I + a K + b K^2 of `rotvec` (a = sin t / t, b = (1 - cos t) / t^2, t = |rotvec|; below t^2 = 1e-6 their Taylor series, so value and
    gradient are finite at rotvec = 0), origins are rotated about the rays' common origin (their mean) and translated.  Pure torch, differentiable with
    respect to `rotvec`, `trans` and the rays; any device."""
    o, d = rays.origins, rays.viewdirs
    rotvec, trans = rotvec.to(d).reshape(3), trans.to(o).reshape(3)
    t2 = (rotvec * rotvec).sum()
    small = t2 < 1e-6
    t2s = torch.where(small, torch.ones_like(t2), t2)      # the branch not taken must not put sqrt'(0) into the gradient
    t = torch.sqrt(t2s)
    a = torch.where(small, 1.0 - t2 / 6.0 + t2 * t2 / 120.0, torch.sin(t) / t)
    b = torch.where(small, 0.5 - t2 / 24.0 + t2 * t2 / 720.0, (1.0 - torch.cos(t)) / t2s)
    zero = torch.zeros_like(t2)
    K = torch.stack([torch.stack([zero, -rotvec[2], rotvec[1]]), torch.stack([rotvec[2], zero, -rotvec[0]]), torch.stack([-rotvec[1], rotvec[0], zero])])
    R = torch.eye(3, dtype=d.dtype, device=d.device) + a * K + b * (K @ K)
    centre = o.detach().reshape(-1, 3).mean(0)
    return Rays((o - centre) @ R.T + centre + trans, d @ R.T)


def allreduce_gradients(parameters, group=None, skip=None):
    """Ray-data-parallel training: every rank renders its own slice of the ray batch, then the gradients of
    the three flat parameter vectors are averaged with one all-reduce each (RCCL over xGMI on GPUs; the hash-table vector
    is 100 MB, the two heads a few KB).  `skip` (device int32 scalar): the per-rank "do not apply this step" flag is summed
    over the ranks as well, so every rank takes the same decision.  No-op without an initialised process group of more
    than one rank.  EVERY rank must call it every step (a rank whose rays produced no sample contributes zero gradients)."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()):
        return
    world = dist.get_world_size(group)
    if world < 2:
        return
    for p_ in parameters:
        if p_.numel() == 0:
            continue                                   # (the reference's `direction_encoding` has no parameters)
        if p_.grad is None:                            # every rank issues the same collectives, whatever its own backward produced
            p_.grad = torch.zeros_like(p_)
        dist.all_reduce(p_.grad, op=dist.ReduceOp.SUM, group=group)
        p_.grad.div_(world)
    if skip is not None:
        dist.all_reduce(skip, op=dist.ReduceOp.SUM, group=group)


# status bits of mnf_train_step's counts_dev[3] (include/mi355nerf.h)
_ST_MARCHED, _ST_ROW, _ST_KEPT, _ST_LABEL, _ST_EMPTY = 1, 2, 4, 8, 16
_ST_GRAD = 32      # mnf_train_render_backward: a non-finite incoming gradient
_STEP_OK, _STEP_ROW, _STEP_GROW = "ok", "row overflow", "bounds overflow; grow"      # what `_step_verdict` says


class TrainState:
    """What train steps keep per FIELD, not per ray count (the reference changes `num_rays` after every iteration, scripts/pipeline.py:494-504, to
    hold the sample count near `target_sample_batch_size`): the sample bounds, the step reports in flight and the counters read from them."""

    def __init__(self):
        self.by_R = {}                          # ray count -> (max_marched, max_kept) raised by synchronous steps of that ray count
        self.abs_m, self.abs_k = 0, 0           # absolute bounds: raised by asynchronous steps and by `reserve`
        self.per_m, self.per_k = 0.0, 0.0       # per-ray bounds: raised by asynchronous steps
        self.pending = []                       # (pinned int64[5], event, ray count) of asynchronous steps whose report has not been read
        self.pinned = []                        # (pinned int64[5], event) pairs free for the next report: at most 3 are in flight
        self.last_counts = None                 # (n_rays, marched, kept) of the latest report read: `latest_step_counts`
        self.skipped_steps = 0                  # asynchronous steps whose final skip flag arrived raised
        self.sched_debt = 0                     # scheduler steps those had been given and the next calls leave out
        self.overflowed_steps = 0               # asynchronous steps that were beyond a sample bound

    def _own(self, R):
        # (the default marched bound has an absolute floor: small batches of the dynamic schedule march ~1000 samples per ray through empty-looking early
        #  grids, and an asynchronous step cannot be repeated; the surviving bound keeps its per-ray form — the deterministic mode's grouping depends on it)
        return self.by_R.get(R, (max(R * 384, 1 << 18), R * 192))

    def caps(self, R):
        """(max_marched, max_kept) of a call with R rays: generous per-ray defaults, raised by what earlier steps of this field overflowed."""
        bm, bk = self._own(R)
        return max(bm, self.abs_m, int(self.per_m * R)), max(bk, self.abs_k, int(self.per_k * R))

    def grow(self, marched, kept, R, carry):
        """Raise the bounds after a step of R rays that overflowed them with `marched` / `kept` samples.
          carry=False (synchronous steps: the overflowing step is repeated at once): only the bounds of this ray count grow — exactly the bounds
                      rounds 1-3 used, which the deterministic mode's partial-sum grouping (and with it the bitwise identity of the stand-in
                      scenes across rounds) depends on;
          carry=True  (asynchronous steps, counts read late): an absolute bound (what the schedule holds constant) and a per-ray bound (what a
                      fixed-size batch holds constant) grow, and every later call — whatever its ray count — uses at least the larger of the two."""
        cm, ck = int(marched * 1.3) + 1024, int(max(kept, marched // 2) * 1.3) + 1024
        if carry:
            self.reserve(cm, ck)
            self.per_m, self.per_k = max(self.per_m, cm / max(R, 1)), max(self.per_k, ck / max(R, 1))
        else:
            bm, bk = self._own(R)
            self.by_R[R] = (max(bm, cm), max(bk, ck))

    def reserve(self, max_marched, max_kept):
        """Every later call, whatever its ray count, is sized for at least these many samples."""
        self.abs_m, self.abs_k = max(self.abs_m, int(max_marched)), max(self.abs_k, int(max_kept))


_TRAIN_STATE = {}


def _train_state(radiance_field) -> TrainState:
    """The field's train state: one per field whatever the ray count of a call (under the reference's schedule it changes every step)."""
    key = id(radiance_field)
    st = _TRAIN_STATE.get(key)
    if st is None:
        st = _TRAIN_STATE[key] = TrainState()
        weakref.finalize(radiance_field, _TRAIN_STATE.pop, key, None)      # (the key holds id(field): drop the entry with the field, or a later field could inherit it)
    return st


def reserve_sample_bounds(radiance_field, max_marched: int, max_kept: int):
    """Raise the field's sample bounds up front: every later train step of this field sizes its launches and workspace for at least `max_marched`
    samples in front of the visibility filter and `max_kept` behind it, whatever its ray count.  For asynchronous training (sync=False), where a step
    beyond its bounds cannot be repeated but is skipped on the device: a caller that knows its budget (`target_sample_batch_size` and the sampler's
    marched / surviving ratio) loses no step to the default per-ray bounds."""
    _train_state(radiance_field).reserve(max_marched, max_kept)


def latest_step_counts(radiance_field):
    """(n_rays, marched samples, surviving samples) of the most recent asynchronous train step of this field whose counts have ARRIVED on the
    host (they travel to pinned memory behind every `sync=False` step and are read at the start of the next call), or None.  What the
    reference's dynamic batch size (scripts/pipeline.py:494-504: num_rays *= target_sample_batch_size / n_rendering_samples) can use
    without waiting for the GPU: the schedule then runs one or two steps behind the counts, the sample bounds absorb the lag."""
    st = _TRAIN_STATE.get(id(radiance_field))
    return None if st is None else st.last_counts


def _step_verdict(marched, kept, longest, status, skipped):
    """What the five host words of a step (marched, kept, longest ray, status, final skip flag) say about it: raises for a label outside the classes,
    else _STEP_ROW (a ray longer than a scratch row: the batch is not one for the fused path), _STEP_GROW (a sample bound was too small) or _STEP_OK."""
    if status & _ST_LABEL:
        raise L.MnfError("train_step: a semantic class id lies outside [0, num_semantic_classes) (F.cross_entropy's device assert)")
    if status & _ST_ROW:
        return _STEP_ROW
    return _STEP_GROW if status & (_ST_MARCHED | _ST_KEPT) else _STEP_OK


def _drain_reports(st, wait):
    """Read the reports of earlier asynchronous steps (`_report_step`): adapt the bounds, surface their errors.  Everything that has arrived is read;
    the step enqueued two calls ago is waited for (the host is at least a step ahead of the GPU: no stall), so a bound that is too small is
    corrected at most two steps late.  `wait`: read them all."""
    while st.pending and (wait or len(st.pending) > 1 or st.pending[0][1].query()):
        host, ev, r_then = st.pending.pop(0)                    # (whatever ray count that step had: the bounds are the field's)
        ev.synchronize()
        c = host.tolist()
        st.pinned.append((host, ev))
        if c[4] > 0:                                            # that step was skipped on the device (no samples, a bound, non-finite gradients): train_step(sync=False)
            st.skipped_steps += 1                               # had already advanced the LR scheduler for it — it owes one scheduler step
            st.sched_debt += 1
        st.last_counts = (r_then, int(c[0]), int(c[1]))         # latest_step_counts(): the dynamic ray-count schedule without a host round trip
        verdict = _step_verdict(*c)
        if verdict == _STEP_ROW:
            raise L.MnfError("train_step: a ray has more samples than a scratch row holds (use the autograd path: fused=False)")
        if verdict == _STEP_GROW:
            st.overflowed_steps += 1
            st.grow(c[0], c[1], r_then, carry=True)


def _report_step(st, out, optimizer=None, wait=False):
    """The five words (`_step_verdict`) of a launched step `out` on their way to a pinned host buffer.  With `optimizer` (an `optim.FusedAdam`) its guarded step is enqueued
    here and its step-count kernel writes them, the final skip flag included; an optimizer not bound to the field, or none, leaves them to copies on the
    stream (no optimizer: the flag is not final, its word stays 0).  wait=True: the host waits and returns them; else `_drain_reports` reads them later."""
    host, ev = st.pinned.pop() if st.pinned else (torch.zeros(5, dtype=torch.int64).pin_memory(), torch.cuda.Event())
    host[4] = 0
    counts, skip = out["counts"], out["skip"]
    if optimizer is not None:
        optimizer.step(skip=skip, count_nonfinite=True, report=(counts, host))
    if optimizer is None or not optimizer.reported:
        host[:4].copy_(counts, non_blocking=True)
        if optimizer is not None:
            host[4:5].copy_(skip.reshape(1).to(torch.int64), non_blocking=True)
    ev.record(torch.cuda.current_stream(counts.device))
    if not wait:
        return st.pending.append((host, ev, out["_rays"]))
    ev.synchronize()
    st.pinned.append((host, ev))
    return host.tolist()


class Presample:
    """A batch's march, done ahead of its train step (`presample`): the C handle, the tensors the march reads and wrote, and what it was made for."""

    def __init__(self):
        h = ctypes.c_void_p()
        L.check(L.load_library().mnf_presample_create(ctypes.byref(h)))
        self.handle = h
        self._box = [None]           # what the march reads and wrote; shared with the finalizer (which must not reference `self`)
        # ONE finalizer does both things in order (a separate __del__ could run after the handle was destroyed at interpreter exit):
        # a token dropped without a step first makes the stream wait for its march — its buffers go back to the allocator only behind it — then the handle goes.
        self._fin = weakref.finalize(self, Presample._drop, L.load_library(), h, self._box)

    @staticmethod
    def _drop(lib, h, box):
        try:
            if box[0] is not None:
                lib.mnf_presample_wait(h, L.stream(box[0][0].device))
        except Exception:
            pass
        box[0] = None
        lib.mnf_presample_destroy(h)

    @property
    def keep(self):
        return self._box[0]

    @keep.setter
    def keep(self, v):
        self._box[0] = v

    def wait(self, device=None):
        """torch's current stream waits for the march (no-op if none was launched or the handle is gone)."""
        if self._fin.alive:
            L.check(L.load_library().mnf_presample_wait(self.handle, L.stream(device)))


def _grid_version(estimator):
    b, o = estimator.binaries, estimator.occs
    return (b.data_ptr(), b._version, o.data_ptr(), o._version)


def _step_seed(presampled, seed):
    """The Philox key of a batch's near-plane jitter: the token's if the batch was presampled, else `seed`, else torch's CPU generator's next draw."""
    if presampled is not None and presampled.keep is not None:
        return presampled.seed
    return int(torch.randint(0, 2 ** 62, (1,)).item()) if seed is None else int(seed)


def _train_opts(radiance_field, grid, device, *, near_plane, far_plane, render_step_size, cone_angle, alpha_thre, stratified, seed, early_stop_eps=0.0,
                loss_scale=0.0, deterministic=False, render_bkgd=None):
    """-> (`mnf_train_opts` of a march or a step, the key under which a presampled march fits a step: the options the march depends on, the
    device copy of `render_bkgd` the options point to, or None).  The march reads the options up to `seed`; `presampled` is left to the launch."""
    opts = L.TrainOpts()
    opts.near_plane, opts.far_plane, opts.render_step_size, opts.cone_angle = near_plane, far_plane, render_step_size, cone_angle
    opts.alpha_thre, opts.early_stop_eps, opts.loss_scale = alpha_thre, early_stop_eps, loss_scale
    opts.stratified = int(radiance_field.training if stratified is None else stratified)
    opts.n_levels, opts.seed = grid.n_levels, seed
    opts.deterministic = int(bool(deterministic))      # bitwise reproducible gradient accumulation (include/mi355nerf.h: mnf_train_opts)
    bk_dev = None
    if render_bkgd is not None and render_bkgd.is_cuda:          # pipeline.py:437 draws the colour on the GPU: hand over the pointer
        bk_dev = L.contig(render_bkgd.detach().reshape(-1)[:3].to(device=device, dtype=torch.float32))
        opts.render_bkgd_dev = bk_dev.data_ptr()
    elif render_bkgd is not None:
        for i, x in enumerate(render_bkgd.detach().reshape(-1)[:3]):
            opts.render_bkgd[i] = float(x)
    key = (float(near_plane), float(far_plane), float(render_step_size), float(cone_angle), float(alpha_thre), int(opts.stratified))
    return opts, key, bk_dev


@torch.no_grad()
def presample(radiance_field, estimator, rays: Rays, near_plane=0.1, far_plane=1e10, render_step_size=1e-3, cone_angle=0.004, alpha_thre=0.01,
              stratified=None, handle: "Presample | None" = None, seed: "int | None" = None):
    """March the NEXT batch now, beside the train step that is enqueued after this call (`mnf_train_presample`, include/mi355nerf.h): the sampler reads
    rays and occupancy grid, not the model, and with one lane per ray it leaves most of the chip idle for ~0.2 ms of every step — the data loader's
    "prefetch the next batch" applied to occ_grid.py:181-208.  Usage, the reference loop of scripts/pipeline.py:447-532 with the batch fetched one
    iteration early:

        tok = None
        for step in range(n):
            # (made in front of step `step`, used by step + 1: worth making only if neither of the two refreshes the occupancy grid)
            nxt = presample(field, est, batches[step + 1].rays, ...) if step % 16 and (step + 1) % 16 else None
            train_step(field, est, opt, *batches[step], step=step, presampled=tok)
            tok = nxt

    Same options as the step's (they are checked).  Call it on the stream the adopting `train_step` will run on (the token's buffers belong to torch's caching
    allocator of that stream; `train_step_ensemble` takes care of its members' streams).  Draws the step's jitter seed from torch's CPU generator, as the step itself would have.  Pass
    `handle` to recycle a consumed `Presample`.  A token that does not fit its step any more (grid refreshed in between, other options) is ignored by
    `train_step`, which then marches itself with the token's seed: results never depend on whether the token was used."""
    if estimator.levels > 4:
        return None
    lib = L.load_library()
    o, d = L.contig(rays.origins.reshape(-1, 3), torch.float32), L.contig(rays.viewdirs.reshape(-1, 3), torch.float32)
    L.require_gpu(o, d)
    R, grid = o.shape[0], _grid_args(estimator)
    opts, key, _ = _train_opts(radiance_field, grid, o.device, near_plane=near_plane, far_plane=far_plane, render_step_size=render_step_size,
                               cone_angle=cone_angle, alpha_thre=alpha_thre, stratified=stratified, seed=_step_seed(None, seed))
    tok = handle if handle is not None else Presample()
    cap_m = _train_state(radiance_field).caps(R)[0]      # the adopting step's bound on marched samples (the march's guard and compaction run here too)
    nbytes = int(lib.mnf_train_presample_workspace_bytes(R, cap_m))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=o.device)
    L.launch(lib.mnf_train_presample, tok.handle, L.ptr(grid.binaries), L.ptr(grid.bits), L.ptr(grid.occs), *grid.res, grid.aabb, L.ptr(o), L.ptr(d), R,
             ctypes.byref(opts), cap_m, L.ptr(ws), nbytes)
    tok.keep = (o, d, ws, grid.binaries, grid.bits)
    tok.seed, tok.R, tok.version, tok.cap_m, tok.key, tok.rays = int(opts.seed), R, _grid_version(estimator), cap_m, key, (rays.origins, rays.viewdirs)
    return tok


REFRESH_EVERY = 16      # the occupancy refresh cadence of `train_step` (pipeline.py:447-470 calls update_every_n_steps with its default n = 16): ONE constant for the refresh
                        # itself, the presample wait in front of a refreshing step, and the batches `presampled_batches` leaves un-presampled


def presampled_batches(batches, radiance_field, estimator, first_step: int = 0, refresh_every: int = REFRESH_EVERY, **render_kw):
    """The reference loop's batches with the march of each one done an iteration early: wraps any iterable of batches (each a tuple or list whose first element is
    the batch's `Rays`) and yields `(step, batch, token)`; pass `presampled=token` to `train_step`.  The next batch is drawn from `batches` and its march enqueued
    (`presample`) BEFORE the current one is yielded, i.e. before the caller enqueues the current step, beside which it then runs.  Batches on either side of an
    occupancy refresh (`step % refresh_every == 0`, as `update_every_n_steps`) are not presampled — their steps march themselves.  `render_kw`: the render
    options the steps will use (near_plane, render_step_size, cone_angle, alpha_thre, stratified).

        for step, (rays, pixels, dep, sem), tok in presampled_batches(loader, field, est, **RENDER_KW):
            train_step(field, est, opt, rays, pixels, dep, sem, bkgd, step=step, sync=False, presampled=tok, **RENDER_KW)"""
    it = iter(batches)
    try:
        cur = next(it)
    except StopIteration:
        return
    if refresh_every != REFRESH_EVERY:
        raise ValueError(f"presampled_batches: train_step refreshes the occupancy grid every {REFRESH_EVERY} steps; a different cadence here would let a refresh "
                         "rewrite the grid under a march in flight")
    step, tok = first_step, None
    while True:
        try:
            nxt = next(it)
        except StopIteration:
            nxt = None
        nxt_tok = None
        if nxt is not None and step % refresh_every and (step + 1) % refresh_every:
            nxt_tok = presample(radiance_field, estimator, nxt[0], **render_kw)
        yield step, cur, tok
        if nxt is None:
            return
        cur, tok, step = nxt, nxt_tok, step + 1


@torch.no_grad()
def _launch_train_step(st, radiance_field, estimator, rays, pixels, dep, sem, render_bkgd, presampled, seed, wait_reports, **opts_kw):
    """Exactly one `mnf_train_step` launch with the field's current sample bounds, behind the reading of earlier steps' reports (`_drain_reports(st,
    wait_reports)`).  `presampled`: the batch's token or None; its march is adopted if it still fits this step (the token is consumed either way).
    Returns `fused_forward_backward`'s dict with the counts as device tensors, which it also leaves in `estimator.last_sampling`."""
    lib = L.load_library()
    o, d = L.contig(rays.origins.reshape(-1, 3), torch.float32), L.contig(rays.viewdirs.reshape(-1, 3), torch.float32)
    live = presampled is not None and presampled.keep is not None
    if live and presampled.rays[0] is rays.origins and presampled.rays[1] is rays.viewdirs:
        o, d = presampled.keep[0], presampled.keep[1]        # (the very tensors the march read: the C side compares pointers)
    L.require_gpu(o, d, pixels, dep, sem)
    R, dev = o.shape[0], o.device
    handle, grid = radiance_field._ensure_handle(), _grid_args(estimator)
    opts, key, bk_dev = _train_opts(radiance_field, grid, dev, seed=seed, loss_scale=float(radiance_field.loss_scale), render_bkgd=render_bkgd, **opts_kw)
    params = [radiance_field.mlp_base.params, radiance_field.mlp_head.params, radiance_field.mlp_sem.params]
    for p_ in params:
        if p_.grad is None or p_.grad.shape != p_.shape or not p_.grad.is_contiguous():
            p_.grad = torch.empty_like(p_)
    tp, td, tl = L.contig(pixels, torch.float32), L.contig(dep, torch.float32), L.contig(sem, torch.int64)
    _drain_reports(st, wait_reports)
    losses, counts, skip = torch.empty(4, device=dev), torch.empty(4, dtype=torch.int64, device=dev), torch.empty((), dtype=torch.int32, device=dev)
    cap_m, cap_k = st.caps(R)
    nbytes = int(lib.mnf_train_step_workspace_bytes(handle, R, cap_m, cap_k))
    ws = _workspace(dev, nbytes)
    # the token's march only if it still fits this step: same rays, grid and options, and the bound on marched samples it was made for
    adopt = (live and presampled.R == R and presampled.keep[0] is o and presampled.version == _grid_version(estimator) and presampled.key == key
             and presampled.cap_m == cap_m)
    if live and not adopt:
        presampled.wait(dev)                                       # (its buffers are released below: not before the march has run)
    opts.presampled = presampled.handle if adopt else None
    L.launch(lib.mnf_train_step, handle, L.ptr(grid.binaries), L.ptr(grid.bits), L.ptr(grid.occs), *grid.res, grid.aabb, L.ptr(o), L.ptr(d), R,
             L.ptr(tp), L.ptr(td), L.ptr(tl), ctypes.byref(opts), L.ptr(params[0].grad), L.ptr(params[1].grad), L.ptr(params[2].grad),
             L.ptr(losses), L.ptr(counts), L.ptr(skip), cap_m, cap_k, L.ptr(ws), nbytes)
    if presampled is not None:
        presampled.adopted = adopt
        presampled.keep = None                                      # consumed (or discarded): the step is enqueued, stream order protects the buffers
    for p_ in params:
        torch.autograd.graph.increment_version(p_.grad)
    estimator.last_sampling = {"n_marched": counts[0]}
    return dict(loss=losses[0], loss_rgb=losses[1], loss_dep=losses[2], loss_sem=losses[3], counts=counts, skip=skip, _keep=bk_dev, _rays=R,
                n_rendering_samples=counts[1], n_marched=counts[0])


def _run_step(batch, presampled, seed, opts_kw, wait_reports, read):
    """A synchronous fused step: `mnf_train_step` is launched, `read(st, out)` enqueues what else belongs to an attempt and brings its five words to
    the host; an attempt beyond its sample bounds changed nothing on the device and is repeated with larger ones (it marches itself: the guards cleared the
    token's counts).  Returns (the launch's result, the words); (None, None) for more than four occupancy levels or a ray longer than a scratch row."""
    st, seed = _train_state(batch[0]), _step_seed(presampled, seed)    # one draw per iteration, whatever the number of attempts
    estimator = batch[1]
    if estimator.levels > 4:
        return None, None
    for attempt in range(4):
        out = _launch_train_step(st, *batch, presampled if attempt == 0 else None, seed, wait_reports, **opts_kw)
        c = read(st, out)                                              # the step's one host round trip, after everything is enqueued
        verdict = _step_verdict(*c)
        if verdict == _STEP_ROW:
            return None, None
        if verdict == _STEP_OK:
            estimator.last_sampling = {"n_marched": int(c[0])}
            out.update(n_rendering_samples=int(c[1]), n_marched=int(c[0]))
            return out, c
        st.grow(c[0], c[1], out["_rays"], carry=False)
    raise L.MnfError("train_step: sample bounds kept growing")


@torch.no_grad()
def fused_forward_backward(radiance_field, estimator, rays: Rays, pixels, dep, sem, render_bkgd=None, near_plane=0.1, far_plane=1e10,
                           render_step_size=1e-3, cone_angle=0.004, alpha_thre=0.01, early_stop_eps=1e-4, stratified=None, sync=True,
                           deterministic=False, presampled: "Presample | None" = None, seed: "int | None" = None):
    """scripts/pipeline.py:472-518 for one model as ONE C call (`mnf_train_step`, csrc/trainstep.hip): train render (occupancy
    sampling + density pre-pass + visibility filter + sem_rendering), the three-term loss and its backward.  Fills `.grad` of
    the three flat parameter vectors.  The call itself never waits for the GPU: the sample counts stay on the device.

    Returns dict(loss, loss_rgb, loss_dep, loss_sem [device scalars], counts [device int64: marched, kept, longest ray, status],
    skip [device int32 scalar: non-zero = the gradients must not be applied], n_rendering_samples, n_marched).
      sync=True   (default) the counts are read back once, AFTER everything is enqueued: n_rendering_samples / n_marched are
                  ints as in the reference; a step whose sample bounds were too small is repeated with larger ones.
      sync=False  nothing is read back: n_rendering_samples / n_marched are 0-d device tensors; the bounds are adapted from the
                  previous call's counts (copied to pinned memory in the background); a step beyond its bounds is skipped on
                  the device (skip != 0) and the bounds grow for the next one.
    Returns None when this estimator / batch cannot take the fused path (more than four occupancy levels, a ray longer than the
    single-pass scratch row): the caller then uses the autograd path, which is the same arithmetic in separate calls."""
    if estimator.levels > 4:
        return None
    batch = (radiance_field, estimator, rays, pixels, dep, sem, render_bkgd)
    opts_kw = dict(near_plane=near_plane, far_plane=far_plane, render_step_size=render_step_size, cone_angle=cone_angle, alpha_thre=alpha_thre,
                   early_stop_eps=early_stop_eps, stratified=stratified, deterministic=deterministic)
    if sync:
        return _run_step(batch, presampled, seed, opts_kw, True, lambda st, out: out["counts"].tolist() + [0])[0]
    st = _train_state(radiance_field)
    out = _launch_train_step(st, *batch, presampled, _step_seed(presampled, seed), False, **opts_kw)
    _report_step(st, out)
    return out


# ------------------------------------------------------------------ the fused step cut at its loss (mnf_train_render_forward / _backward)
_LAST_RENDER = weakref.WeakKeyDictionary()      # field -> the device counters and skip flag of its latest `fused_train_render` (`latest_train_render`)


def latest_train_render(radiance_field):
    """dict(counts [device int64: marched, kept, longest ray, status], skip [device int32 scalar]) of the field's most recent `fused_train_render`, or None if that
    call handed over to `render_image_with_occgrid_with_depth_guide` (or none was made).  The backward of that render adds to them: status bit 32 and a raised
    flag for a non-finite incoming gradient.  `skip` is what a guarded optimizer step takes (`optim.FusedAdam.step(skip=...)`)."""
    return _LAST_RENDER.get(radiance_field)


def _param_versions(radiance_field):
    ps = (radiance_field.mlp_base.params, radiance_field.mlp_head.params, radiance_field.mlp_sem.params)
    return tuple(p._version for p in ps) + (ps[0].data_ptr(),)


@torch.no_grad()
def _launch_train_render(st, radiance_field, estimator, rays, render_bkgd, seed, own_workspace, **opts_kw):
    """Exactly one `mnf_train_render_forward` launch with the field's current sample bounds.  `own_workspace`: the call's scratch is a tensor of its own (a
    differentiable call: its backward reads it, whatever runs in between) instead of the cached slot the next call overwrites.  Returns the four planes, the
    device counters and skip flag, and what the backward needs."""
    lib = L.load_library()
    o, d = L.contig(rays.origins.reshape(-1, 3), torch.float32), L.contig(rays.viewdirs.reshape(-1, 3), torch.float32)
    L.require_gpu(o, d)
    R, dev, C = o.shape[0], o.device, radiance_field.num_semantic_classes
    handle, grid = radiance_field._ensure_handle(), _grid_args(estimator)
    if own_workspace and render_bkgd is not None and render_bkgd.is_cuda:
        render_bkgd = render_bkgd.detach().clone()      # the backward reads the colour again: the forward's three floats, whatever the caller draws into its tensor meanwhile
    opts, _, bk_dev = _train_opts(radiance_field, grid, dev, seed=seed, loss_scale=float(radiance_field.loss_scale), render_bkgd=render_bkgd, **opts_kw)
    counts, skip = torch.empty(4, dtype=torch.int64, device=dev), torch.empty((), dtype=torch.int32, device=dev)
    rgb, acc, depth, sem = torch.empty(R, 3, device=dev), torch.empty(R, 1, device=dev), torch.empty(R, 1, device=dev), torch.empty(R, C, device=dev)
    cap_m, cap_k = st.caps(R)
    nbytes = int(lib.mnf_train_step_workspace_bytes(handle, R, cap_m, cap_k))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev) if own_workspace else _workspace(dev, nbytes)
    L.launch(lib.mnf_train_render_forward, handle, L.ptr(grid.binaries), L.ptr(grid.bits), L.ptr(grid.occs), *grid.res, grid.aabb, L.ptr(o), L.ptr(d), R,
             ctypes.byref(opts), L.ptr(rgb), L.ptr(acc), L.ptr(depth), L.ptr(sem), L.ptr(counts), L.ptr(skip), cap_m, cap_k, L.ptr(ws), nbytes)
    return dict(rgb=rgb, acc=acc, depth=depth, sem=sem, counts=counts, skip=skip, _rays=R, _field=radiance_field, _handle=handle, _opts=opts, _keep=bk_dev,
                _dirs=d if own_workspace else None,      # the contiguous fp32 [R,3] directions the kernels read: a ray-gradient backward reads them again
                _caps=(cap_m, cap_k), _ws=ws if own_workspace else None, _nbytes=nbytes, _versions=radiance_field._loaded_versions)


def _train_render_backward(call, grads_out, want_params, want_o=False, want_d=False):
    """The backward both autograd nodes of `fused_train_render` share: `mnf_train_render_backward`, or — when a ray gradient is asked for —
    `mnf_train_render_backward_rays`, with whatever gradients autograd delivered (None as NULL, strides passed through, no `.contiguous()`).
    `want_params` False: the parameter pointers go in as NULL (frozen: no weight gradients, no hash scatter).  -> (three parameter gradients | None, g_o, g_d)."""
    field = call["_field"]
    if call["_ws"] is None:
        raise L.MnfError("fused_train_render: a second backward through the same render (its backward overwrites the workspace the first one read); "
                         "render again")
    if field._loaded_versions != call["_versions"] or _param_versions(field) != call["_versions"]:
        raise L.MnfError("fused_train_render: the field's parameters changed between the render and its backward (an optimizer step, a load): the 16-bit "
                         "weights in the handle are no longer the forward's")
    params = (field.mlp_base.params, field.mlp_head.params, field.mlp_sem.params)
    grads = [torch.empty_like(p_, memory_format=torch.contiguous_format) for p_ in params] if want_params else None
    dev, R = call["counts"].device, call["_rays"]
    gs = [None if g is None else g.to(device=dev, dtype=torch.float32) for g in grads_out]      # (no-ops: autograd delivers fp32 on the device)
    st0 = lambda g: 0 if g is None else g.stride(0)
    st1 = lambda g: 0 if g is None else g.stride(1)
    ws, call["_ws"] = call["_ws"], None
    lib = L.load_library()
    g_in = (L.ptr(gs[0]), st0(gs[0]), st1(gs[0]), L.ptr(gs[1]), st0(gs[1]), L.ptr(gs[2]), st0(gs[2]), L.ptr(gs[3]), st0(gs[3]), st1(gs[3]))
    g_par = tuple(L.ptr(g) for g in grads) if want_params else (None, None, None)
    tail = (L.ptr(call["counts"]), L.ptr(call["skip"]), *call["_caps"], L.ptr(ws), call["_nbytes"])
    g_o = g_d = None
    if want_o or want_d:
        g_o = torch.empty(R, 3, device=dev) if want_o else None
        g_d = torch.empty(R, 3, device=dev) if want_d else None
        L.launch(lib.mnf_train_render_backward_rays, call["_handle"], R, ctypes.byref(call["_opts"]), L.ptr(call["_dirs"]), *g_in, *g_par, L.ptr(g_o), L.ptr(g_d),
                 *tail)
    else:
        L.launch(lib.mnf_train_render_backward, call["_handle"], R, ctypes.byref(call["_opts"]), *g_in, *g_par, *tail)
    return grads, g_o, g_d


class _TrainRender(torch.autograd.Function):
    """The autograd node of `fused_train_render`: inputs the three flat parameter vectors, outputs the four rendered planes of a launched
    `mnf_train_render_forward` (`call`), backward `mnf_train_render_backward` with whatever gradients autograd delivers — None as NULL, strides passed
    through, no `.contiguous()`."""

    @staticmethod
    def forward(ctx, call, p_base, p_head, p_sem):
        planes = tuple(call.pop(k) for k in ("rgb", "acc", "depth", "sem"))      # (not kept: the planes own this node, the node must not own the planes)
        ctx.call = call
        ctx.set_materialize_grads(False)      # a plane the loss does not use arrives as None (-> NULL), not as a zero tensor
        return planes

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_rgb, g_acc, g_depth, g_sem):
        grads, _, _ = _train_render_backward(ctx.call, (g_rgb, g_acc, g_depth, g_sem), True)
        return None, grads[0], grads[1], grads[2]


class _TrainRenderRays(torch.autograd.Function):
    """`_TrainRender` with `rays.origins` and `rays.viewdirs` as inputs besides the three parameter vectors (`fused_train_render_rays`): its
    backward is `mnf_train_render_backward_rays`, asked only for what `ctx.needs_input_grad` wants — the parameter pointers NULL when no parameter requires
    a gradient — and returns the ray gradients in the shape and dtype of the tensors it was given.  The sample set is a constant of the render."""

    @staticmethod
    def forward(ctx, call, origins, viewdirs, p_base, p_head, p_sem):
        planes = tuple(call.pop(k) for k in ("rgb", "acc", "depth", "sem"))
        ctx.call = call
        ctx.ray_meta = ((origins.shape, origins.dtype), (viewdirs.shape, viewdirs.dtype))
        ctx.set_materialize_grads(False)
        return planes

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_rgb, g_acc, g_depth, g_sem):
        need = ctx.needs_input_grad
        grads, g_o, g_d = _train_render_backward(ctx.call, (g_rgb, g_acc, g_depth, g_sem), any(need[3:6]), need[1], need[2])
        g_rays = tuple(None if g is None else g.view(shape).to(dtype) for g, (shape, dtype) in zip((g_o, g_d), ctx.ray_meta))
        g_params = tuple(g if w else None for g, w in zip(grads, need[3:6])) if grads is not None else (None, None, None)
        return (None,) + g_rays + g_params


def fused_train_render(radiance_field, estimator, rays: Rays, near_plane: float = 0.0, far_plane: float = 1e10, render_step_size: float = 1e-3,
                       render_bkgd: Optional[torch.Tensor] = None, cone_angle: float = 0.0, alpha_thre: float = 0.0, early_stop_eps: float = 1e-4,
                       depth: Optional[torch.Tensor] = None, stratified=None, seed: "int | None" = None, deterministic: bool = False):
    """`render_image_with_occgrid_with_depth_guide` (utils.py:63-219) on the kernels of the one-call train step, differentiable with respect to the field's
    parameters: any torch loss on the returned planes, then `loss.backward()`, runs the step's own forward and backward (`mnf_train_render_forward` /
    `mnf_train_render_backward`) around it.  Switching over is the import line

        from apnrf_amd.render import fused_train_render as render_image_with_occgrid_with_depth_guide

    Returns (rgb [..,3], acc [..,1], depth [..,1], sem [..,C], n_rendering_samples: int) as the drop-in does.  `depth` is accepted and ignored, as in the
    reference; `stratified=None` follows `radiance_field.training`; `seed`: the Philox key of the near-plane jitter (None: torch's CPU generator's next draw);
    `deterministic=True`: bitwise reproducible gradient accumulation.  One host round trip (the four counters: the `int` the reference returns demands it); a
    render beyond its sample bounds is repeated with larger ones (it is pure).  More than four occupancy levels, or a ray past the sampler's scratch row, hand
    over to `render_image_with_occgrid_with_depth_guide`; the hand-over follows `radiance_field.training` as the drop-in does: `stratified=False` is honoured
    (the field is put into eval mode for the call), `stratified=True` on a field in eval mode is not, and the drop-in has no `early_stop_eps`, `seed` or
    `deterministic` to pass on.  So does a call whose `rays.origins` or `rays.viewdirs` requires a gradient (with autograd on): the drop-in returns the ray
    gradients; `fused_train_render_rays` is the same call kept on the fused route.
    One backward per render, and the parameters must not change between the two (both raise `MnfError`).  Under `torch.no_grad()`, or with no parameter
    requiring a gradient, nothing is kept for a backward.  `latest_train_render(radiance_field)` has the device counters and the skip flag."""
    return _fused_train_render(radiance_field, estimator, rays, False, near_plane, far_plane, render_step_size, render_bkgd, cone_angle, alpha_thre,
                               early_stop_eps, depth, stratified, seed, deterministic)


def fused_train_render_rays(radiance_field, estimator, rays: Rays, near_plane: float = 0.0, far_plane: float = 1e10, render_step_size: float = 1e-3,
                            render_bkgd: Optional[torch.Tensor] = None, cone_angle: float = 0.0, alpha_thre: float = 0.0, early_stop_eps: float = 1e-4,
                            depth: Optional[torch.Tensor] = None, stratified=None, seed: "int | None" = None, deterministic: bool = False):
    """`fused_train_render` — same arguments, same five results, same bookkeeping — for a caller who differentiates with respect to the RAYS: a call whose
    `rays.origins` or `rays.viewdirs` requires a gradient (with autograd on) stays on the fused route instead of handing over.  Its backward
    (`mnf_train_render_backward_rays`) returns dL/d(`rays.origins`) and dL/d(`rays.viewdirs`), in the shape and dtype of the tensors given, beside — or, with
    every parameter frozen, instead of — the parameter gradients; with frozen parameters it launches no weight gradient and no hash-table scatter (pose
    refinement behind `transform_rays`: INTEGRATION.md §A).  The sample set is a constant of the render, as on the drop-in route; no gradient reaches the
    distances or the background colour.  Without a ray that requires a gradient it is `fused_train_render`; more than four occupancy levels or a ray past
    the scratch row still hand over (the drop-in returns the ray gradients there)."""
    return _fused_train_render(radiance_field, estimator, rays, True, near_plane, far_plane, render_step_size, render_bkgd, cone_angle, alpha_thre,
                               early_stop_eps, depth, stratified, seed, deterministic)


def _fused_train_render(radiance_field, estimator, rays, ray_gradients, near_plane, far_plane, render_step_size, render_bkgd, cone_angle, alpha_thre,
                        early_stop_eps, depth, stratified, seed, deterministic):
    """What `fused_train_render` (`ray_gradients` False: rays that require a gradient hand over) and `fused_train_render_rays` (True) share"""
    _LAST_RENDER.pop(radiance_field, None)

    def hand_over():
        no_jitter = stratified is False and radiance_field.training      # (the drop-in's jitter follows radiance_field.training: `_train_autograd`)
        if no_jitter:
            radiance_field.eval()
        try:
            return render_image_with_occgrid_with_depth_guide(radiance_field, estimator, rays, near_plane=near_plane, far_plane=far_plane,
                                                              render_step_size=render_step_size, render_bkgd=render_bkgd, cone_angle=cone_angle,
                                                              alpha_thre=alpha_thre, depth=depth)
        finally:
            if no_jitter:
                radiance_field.train()

    if estimator.levels > 4 or rays.origins.numel() == 0:
        return hand_over()
    want_rays = torch.is_grad_enabled() and (rays.origins.requires_grad or rays.viewdirs.requires_grad)
    if want_rays and not ray_gradients:
        return hand_over()      # gradients of the rays: the drop-in delivers them (`sem_rendering`); the fused route does for `fused_train_render_rays` only
    st, seed = _train_state(radiance_field), _step_seed(None, seed)      # one draw per render, whatever the number of attempts
    differentiable = torch.is_grad_enabled() and (want_rays or any(p_.requires_grad for p_ in radiance_field.parameters()))
    opts_kw = dict(near_plane=near_plane, far_plane=far_plane, render_step_size=render_step_size, cone_angle=cone_angle, alpha_thre=alpha_thre,
                   early_stop_eps=early_stop_eps, stratified=stratified, deterministic=deterministic)
    for attempt in range(4):
        out = _launch_train_render(st, radiance_field, estimator, rays, render_bkgd, seed, differentiable, **opts_kw)
        c = out["counts"].tolist()                                        # the render's one host round trip
        verdict = _step_verdict(*c, 0)
        if verdict == _STEP_ROW:
            return hand_over()
        if verdict == _STEP_OK:
            break
        st.grow(c[0], c[1], out["_rays"], carry=False)
    else:
        raise L.MnfError("fused_train_render: sample bounds kept growing")
    estimator.last_sampling = {"n_marched": int(c[0])}
    _LAST_RENDER[radiance_field] = dict(counts=out["counts"], skip=out["skip"])
    if want_rays:
        planes = _TrainRenderRays.apply(out, rays.origins, rays.viewdirs, radiance_field.mlp_base.params, radiance_field.mlp_head.params,
                                        radiance_field.mlp_sem.params)
    elif differentiable:
        planes = _TrainRender.apply(out, radiance_field.mlp_base.params, radiance_field.mlp_head.params, radiance_field.mlp_sem.params)
    else:
        planes = (out["rgb"], out["acc"], out["depth"], out["sem"])
    shp = tuple(rays.origins.shape[:-1])
    return tuple(x.view(*shp, -1) for x in planes) + (int(c[1]),)


def _step_result(fwd, skipped, sync):
    """`train_step`'s result.  A synchronous step without a surviving sample is the reference's `continue` (pipeline.py:491): no loss."""
    if sync and fwd["n_rendering_samples"] == 0:
        return dict(loss=None, n_rendering_samples=0, skipped=True)
    det = lambda x: None if x is None else x.detach()      # (a caller's `loss_fn` has no terms to report)
    return dict(loss=det(fwd["loss"]), loss_rgb=det(fwd["loss_rgb"]), loss_dep=det(fwd["loss_dep"]), loss_sem=det(fwd["loss_sem"]),
                n_rendering_samples=fwd["n_rendering_samples"], skipped=skipped)


def _train_fused_one_trip(batch, optimizer, scheduler, presampled, seed, opts_kw):
    """The reference's loop form (n_rendering_samples and the skip decision on the host after every iteration) with ONE host round trip and no bubble on
    the GPU: render + loss + backward AND the guarded optimizer call are enqueued first, then the host waits once for the five words the optimizer's
    step-count kernel wrote into pinned memory.  A step beyond its sample bounds has raised the flag on the device: its optimizer call changed
    nothing, the bounds grow and the step is repeated.  None: the batch is not one for the fused path (the flagged optimizer call changed nothing)."""
    out, c = _run_step(batch, presampled, seed, opts_kw, False, lambda st, out: _report_step(st, out, optimizer, wait=True))
    if out is None:
        return None
    skipped = c[4] > 0
    if not skipped and scheduler is not None:
        scheduler.step()
    return _step_result(out, skipped, True)


def _apply_update(radiance_field, optimizer, scheduler, fwd, sync, data_parallel, data_parallel_group):
    """pipeline.py:520-532 behind a forward + backward `fwd` (its losses, `skip` flag and `n_rendering_samples`): gradient all-reduce, non-finite
    guard, optimizer and scheduler step; returns `train_step`'s result."""
    from .optim import FusedAdam, count_nan_gradients
    skip = fwd["skip"]
    if data_parallel:
        allreduce_gradients(radiance_field.parameters(), data_parallel_group, skip)
    if not sync:
        # the step's counters and its FINAL skip flag (the optimizer's non-finite guard included) travel to pinned host memory; when they arrive — one or two
        # calls later — a skipped step takes back the scheduler step it is given here: the schedule counts optimizer updates, as pipeline.py:491 / :520-532 do
        st = _train_state(radiance_field)
        if "counts" in fwd:                                                    # a fused step: the optimizer call reports it
            _report_step(st, fwd, optimizer)
        else:
            optimizer.step(skip=skip, count_nonfinite=True)
        if scheduler is not None and st.sched_debt > 0:
            st.sched_debt -= 1
        elif scheduler is not None:
            scheduler.step()
        return _step_result(fwd, skip, False)
    if isinstance(optimizer, FusedAdam):
        # the non-finite count is added to the same flag and the update leaves everything untouched when it is raised — one C call for guard + three
        # updates + handle refresh when the optimizer is bound to the field (`bind_field`)
        optimizer.step(skip=skip, count_nonfinite=True)
        skipped = bool(skip.item() > 0)                                        # one host round trip per iteration
    else:
        count_nan_gradients(radiance_field.parameters(), out=skip)             # pipeline.py:520-529
        skipped = bool(skip.item() > 0)
        optimizer.zero_grad() if skipped else optimizer.step()
    if not skipped and scheduler is not None:
        scheduler.step()
    return _step_result(fwd, skipped, True)


def _train_fused(batch, optimizer, scheduler, sync, data_parallel, data_parallel_group, presampled, seed, opts_kw):
    """The fused forward + backward followed by `_apply_update`: synchronous steps of a data-parallel run or a host-stepped optimizer (two round
    trips), and every asynchronous step (none).  None: the batch is not one for the fused path."""
    if batch[1].levels > 4:
        return None
    if sync:
        fwd = fused_forward_backward(*batch, presampled=presampled, seed=seed, **opts_kw)
    else:
        fwd = _launch_train_step(_train_state(batch[0]), *batch, presampled, _step_seed(presampled, seed), False, **opts_kw)
    return None if fwd is None else _apply_update(batch[0], optimizer, scheduler, fwd, sync, data_parallel, data_parallel_group)


def _train_autograd(batch, optimizer, scheduler, sync, data_parallel, data_parallel_group, stratified, **render_kw):
    """The differentiable Python surface (`render_image_with_occgrid_with_depth_guide` + torch losses + autograd): fused=False, or a batch the fused call
    handed over (more than four occupancy levels / a ray past the sampler's scratch row).  The reference's signature has no jitter switch (it follows
    radiance_field.training, occ_grid.py:187-189): `stratified=False` is honoured by rendering in eval mode."""
    import torch.nn.functional as F
    radiance_field, estimator, rays, pixels, dep, sem, render_bkgd = batch
    no_jitter = stratified is False and radiance_field.training
    if no_jitter:
        radiance_field.eval()
    try:
        rgb, acc, depth, semantic, n_rendering_samples = render_image_with_occgrid_with_depth_guide(
            radiance_field, estimator, rays, render_bkgd=render_bkgd, depth=dep, **render_kw)
    finally:
        if no_jitter:
            radiance_field.train()
    dev = rays.origins.device
    skip = torch.zeros((), dtype=torch.int32, device=dev)      # device flag: raised for a step without samples
    optimizer.zero_grad()
    if n_rendering_samples == 0:
        # pipeline.py:491: `continue`.  With data_parallel the collective still has to be reached by this rank:
        # it contributes zero gradients and a raised skip flag.
        skip += 1
        for p_ in radiance_field.parameters():
            if p_.numel():
                p_.grad = torch.zeros_like(p_)
        loss = loss_rgb = loss_dep = loss_sem = torch.zeros((), device=dev)
    else:
        loss_rgb = F.smooth_l1_loss(rgb, pixels)
        loss_dep = F.smooth_l1_loss(depth, dep.unsqueeze(1))
        loss_sem = F.cross_entropy(semantic, sem)
        loss = loss_rgb * 10 + loss_dep / 5 + loss_sem / 2
        loss.backward()
    fwd = dict(loss=loss, loss_rgb=loss_rgb, loss_dep=loss_dep, loss_sem=loss_sem, skip=skip, n_rendering_samples=n_rendering_samples)
    return _apply_update(radiance_field, optimizer, scheduler, fwd, sync, data_parallel, data_parallel_group)


def _train_loss_fn(batch, optimizer, scheduler, loss_fn, data_parallel, data_parallel_group, stratified, seed, deterministic, **render_kw):
    """`train_step(loss_fn=...)`: `fused_train_render` -> the caller's loss -> `backward()` -> `_apply_update`.  The render's device skip flag (no surviving sample;
    after the backward also a non-finite incoming gradient) is the one the guarded optimizer call reads."""
    radiance_field, estimator, rays, pixels, dep, sem, render_bkgd = batch
    rgb, acc, depth, semantic, n_rendering_samples = fused_train_render(radiance_field, estimator, rays, render_bkgd=render_bkgd, depth=dep, stratified=stratified,
                                                                        seed=seed, deterministic=deterministic, **render_kw)
    dev = rays.origins.device
    last = latest_train_render(radiance_field)      # (None: the render was handed over to the call-by-call surface)
    skip = last["skip"] if last is not None else torch.zeros((), dtype=torch.int32, device=dev)
    optimizer.zero_grad()
    if n_rendering_samples == 0:                    # pipeline.py:491: `continue`; a data-parallel rank still reaches the collective, with zero gradients
        if last is None:
            skip += 1
        for p_ in radiance_field.parameters():
            if p_.numel():
                p_.grad = torch.zeros_like(p_)
        loss = torch.zeros((), device=dev)
    else:
        loss = loss_fn(rgb, acc, depth, semantic, pixels, dep, sem)
        loss.backward()
    fwd = dict(loss=loss, loss_rgb=None, loss_dep=None, loss_sem=None, skip=skip, n_rendering_samples=n_rendering_samples)
    return _apply_update(radiance_field, optimizer, scheduler, fwd, True, data_parallel, data_parallel_group)


def train_step(radiance_field, estimator, optimizer, rays: Rays, pixels, dep, sem, render_bkgd, step: int,
               near_plane=0.1, render_step_size=1e-3, cone_angle=0.004, alpha_thre=0.01, occ_thre=1e-3, scheduler=None,
               data_parallel_group=None, data_parallel=False, fused=True, sync=True, stratified=None, deterministic=False, presampled=None, seed=None,
               loss_fn=None):
    """One model's training iteration exactly as scripts/pipeline.py:447-532 sequences it: occupancy refresh every 16th
    step (:447-470), train render (:472-489), loss 10*smoothL1(rgb) + smoothL1(depth)/5 + CE(sem)/2 (:506-511),
    backward (:518), NaN-gradient guard (:520-529), optimizer and scheduler step (:531-532).  `data_parallel=True`
    averages the gradients (and sums the skip flags) over the ranks of `data_parallel_group` before the guard (each rank holds
    a slice of the rays; every rank reaches the collective every step, whatever its own batch produced).
    `fused=True` (default) runs render + loss + backward as one C call (`fused_forward_backward`); `fused=False` goes through
    the differentiable Python surface (`render_image_with_occgrid_with_depth_guide` + torch losses + autograd), which is the
    same kernels call by call.

    With `optim.FusedAdam` the decision "skip this iteration" (no surviving sample, non-finite gradient) is taken on the
    device and the iteration is enqueued without waiting for the GPU:
      sync=True   (default) ONE host round trip, behind the enqueued optimizer call (the reference has one per parameter plus two inside the sampler):
                  returns n_rendering_samples as an int and skipped as a bool, steps the scheduler only if the optimizer stepped.
      sync=False  no round trip at all: n_rendering_samples and skipped are device tensors; the scheduler advances every call, and a step whose skip
                  flag arrives raised (one or two calls later, with its counts) gives its scheduler step back: the schedule counts optimizer updates.
    Any other optimizer is stepped from the host after reading the flag (sync=True only).
    `stratified` (fused path): None = jitter the near planes as the reference does in training mode (occ_grid.py:187-189);
    False = no jitter (reproducible sample sets: parity tests).  `deterministic=True` (fused path): gradients are accumulated in an
    order-independent way (64-bit fixed-point integer atomics for the hash table, ordered partial sums for the weights): with a
    seeded torch generator the whole training run is bitwise reproducible.
    `seed` (fused path): the Philox key of the near-plane jitter (None: torch's CPU generator's next draw).
    `presampled` (fused path): the `presample()` token of THIS batch — its march ran beside the previous iteration; ignored (the step marches itself,
    with the token's jitter seed) if the occupancy refresh below or other options made it stale.
    `loss_fn` (sync=True only): a callable `loss_fn(rgb, acc, depth, sem, pixels, dep, sem_gt) -> scalar` replaces the three-term loss; the iteration then runs
    `fused_train_render` -> `loss_fn` -> `backward()` on the same kernels (the result's loss_rgb / loss_dep / loss_sem are None).  None: nothing changes.
    Returns dict(loss, loss_rgb, loss_dep, loss_sem as device tensors, n_rendering_samples, skipped)."""
    from .optim import FusedAdam
    if loss_fn is not None and not sync:
        raise ValueError("train_step(loss_fn=...) is synchronous: the render returns n_rendering_samples as an int (sync=False is the built-in loss's)")
    radiance_field.train()
    estimator.train()
    if presampled is not None and presampled.keep is not None and step % REFRESH_EVERY == 0:
        # only a step that refreshes the grid (update_every_n_steps: step % 16 == 0) needs the march finished before it starts: the refresh must not rewrite the
        # grid under it.  Every other step leaves the wait to mnf_train_step, which skips it when hipEventQuery says the march is done (a cross-queue wait costs
        # the stream ~18 us even then; ADVICE r04: waiting here unconditionally made that shortcut dead).
        presampled.wait(rays.origins.device)
    device_guard = isinstance(optimizer, FusedAdam)
    if not sync and not (fused and device_guard):
        raise ValueError("train_step(sync=False) needs fused=True and optim.FusedAdam (the skip decision is taken on the device)")

    occ_eval_fn = NA.FieldDensityOcc(radiance_field, render_step_size)     # pipeline.py:376-378; one fused C call per refresh
    estimator.update_every_n_steps(step=step, occ_eval_fn=occ_eval_fn, occ_thre=occ_thre, n=REFRESH_EVERY)
    batch = (radiance_field, estimator, rays, pixels, dep, sem, render_bkgd)
    render_kw = dict(near_plane=near_plane, render_step_size=render_step_size, cone_angle=cone_angle, alpha_thre=alpha_thre)
    opts_kw = dict(render_kw, far_plane=1e10, early_stop_eps=1e-4, stratified=stratified, deterministic=deterministic)
    if loss_fn is not None:
        if presampled is not None:
            presampled.wait(rays.origins.device)      # (presample adoption is the one-call step's: the token is left unused, its buffers behind its march)
        return _train_loss_fn(batch, optimizer, scheduler, loss_fn, data_parallel, data_parallel_group, stratified, seed, deterministic, **render_kw)
    if fused and sync and device_guard and not data_parallel:
        res = _train_fused_one_trip(batch, optimizer, scheduler, presampled, seed, opts_kw)
    else:
        res = _train_fused(batch, optimizer, scheduler, sync, data_parallel, data_parallel_group, presampled, seed, opts_kw) if fused else None
    return res if res is not None else _train_autograd(batch, optimizer, scheduler, sync, data_parallel, data_parallel_group, stratified, **render_kw)


_ENSEMBLE_STREAMS = {}


def ensemble_streams(device, n: int):
    """The streams an ensemble's members train on: the caller's current stream for member 0, one cached extra stream per further member (created
    once per device and kept: the platform dislikes processes that keep creating streams)."""
    device = torch.device(device)
    extra = _ENSEMBLE_STREAMS.setdefault(device, [])
    while len(extra) < n - 1:
        extra.append(torch.cuda.Stream(device))
    return [torch.cuda.current_stream(device)] + extra[:max(n - 1, 0)]


def train_step_ensemble(members, batches, step: int, **kw):
    """One iteration of the reference's ensemble (scripts/pipeline.py:398-412 trains the members ONE AFTER THE OTHER inside every iteration; they are
    independent models): every member's `train_step(sync=False)` is enqueued on a stream of its own, so that the latency-bound phases of one member's
    step (the ray marcher, the small launches, the tail of each kernel) run beside the other member's kernels — at the reference yaml's 2000 rays a
    single step cannot fill 256 compute units (measured: 1.55 -> 1.15 ms per member step with two members, profiles/r04_exp_ensemble.txt).
    `members`: list of (radiance_field, estimator, optimizer[, scheduler]) with `optim.FusedAdam` optimizers (the skip decision is taken on the device);
    `batches`: one (rays, pixels, dep, sem, render_bkgd) per member.  Inputs may have been produced on the caller's stream; on return the caller's stream
    waits for every member.  Results are those of the members stepped one after the other (they share nothing).  Returns the members' result dicts."""
    assert len(members) == len(batches) and len(members) >= 1
    tokens = kw.pop("presampled", None) or [None] * len(members)      # one `presample()` token per member (made on the caller's stream), or None
    dev = batches[0][0].origins.device
    streams = ensemble_streams(dev, len(members))
    cur = streams[0]
    ready = torch.cuda.Event()
    ready.record(cur)
    outs = []
    for m, (member, (rays, pixels, dep, sem, bkgd)) in enumerate(zip(members, batches)):
        field, est, opt = member[:3]
        sched = member[3] if len(member) > 3 else None
        s_ = streams[m]
        if m:
            s_.wait_event(ready)                       # whatever produced this member's inputs on the caller's stream comes first
            for t in (rays.origins, rays.viewdirs, pixels, dep, sem, bkgd) + tuple((tokens[m].keep or ())[:3] if tokens[m] is not None else ()):
                if isinstance(t, torch.Tensor) and t.is_cuda:
                    t.record_stream(s_)                 # the caching allocator must not hand the inputs' memory out again before this stream has read it
        with torch.cuda.stream(s_):
            outs.append(train_step(field, est, opt, rays, pixels, dep, sem, bkgd, step=step, scheduler=sched, sync=False, presampled=tokens[m], **kw))
    for s_ in streams[1:]:
        cur.wait_stream(s_)
    return outs


# ------------------------------------------------------------------ habitat_to_data.py
def pose_to_c2w(p: np.ndarray) -> np.ndarray:
    """habitat_to_data.py:444-451: xyz + quaternion (x, y, z, w) -> 4x4 camera-to-world (float64 on the host)."""
    from scipy.spatial.transform import Rotation as R
    pose = np.eye(4)
    pose[:3, :3] = R.from_quat(p[3:]).as_matrix()
    pose[:3, 3] = p[:3]
    return pose


def subsample_indices(n_total: int, n_keep: int) -> np.ndarray:
    """habitat_to_data.py:462-467 (np.round = half-to-even, evaluated in float64 on the host)."""
    return np.round(np.linspace(0, n_total - 1, n_keep)).astype(np.int64)


@torch.no_grad()
def generate_image_rays(pose, width, height, K, device, pix_idx=None):
    """Dataset.generate_image_rays (habitat_to_data.py:274-301) for `pose` [V,4,4] / [V,3,4]; K is the 3x3
    intrinsics the reference builds (only K[0,0] is used, fx == fy, principal point = image centre).
    With `pix_idx` only those flat pixel indices are generated (the reference builds all W*H rays and then indexes)."""
    pose = torch.as_tensor(np.asarray(pose.detach().cpu()) if isinstance(pose, torch.Tensor) else np.asarray(pose), dtype=torch.float32)
    c2w = pose[:, :3, :4].contiguous().to(device)
    L.require_gpu(c2w)
    K = np.asarray(K.detach().cpu()) if isinstance(K, torch.Tensor) else np.asarray(K)
    if abs(K[0, 2] - width / 2) > 1e-9 or abs(K[1, 2] - height / 2) > 1e-9 or abs(K[0, 0] - K[1, 1]) > 1e-9:
        raise NotImplementedError("generate_image_rays supports the reference intrinsics (fx == fy, centred principal point)")
    V = c2w.shape[0]
    idx_t = None
    n_pix = width * height
    if pix_idx is not None:
        idx_t = torch.as_tensor(np.asarray(pix_idx), dtype=torch.int64).to(device)
        n_pix = idx_t.shape[0]
    origins = torch.empty(V, n_pix, 3, device=device)
    viewdirs = torch.empty(V, n_pix, 3, device=device)
    L.launch(L.load_library().mnf_generate_rays, L.ptr(c2w), V, width, height, float(np.float32(K[0, 0])), L.ptr(idx_t), n_pix,
                                               L.ptr(origins), L.ptr(viewdirs))
    if V == 1:
        return Rays(origins=origins[0], viewdirs=viewdirs[0])
    return Rays(origins=origins, viewdirs=viewdirs)


def _pose_rays(poses, width, height, focal, scale, device):
    c2w = np.stack([pose_to_c2w(np.asarray(p, np.float64)) for p in poses]).astype(np.float32)
    h, w = int(height * scale), int(width * scale)
    idx = subsample_indices(width * height, h * w)
    K = np.array([[focal, 0.0, width / 2], [0.0, focal, height / 2], [0.0, 0.0, 1.0]])
    rays = generate_image_rays(torch.from_numpy(c2w), width, height, K, device, idx)
    V = c2w.shape[0]
    return rays.origins.reshape(V * h * w, 3), rays.viewdirs.reshape(V * h * w, 3), h, w


def _host_stacks_f64(outputs):
    """The float64 host arrays the reference's drivers return (habitat_to_data.py:376-409, :497-544: `np.zeros(...)` stacks filled from `.cpu().numpy()`), made
    with ONE device-to-host transfer: every output is widened to float64 on the device and lands in one pinned block (torch's caching host allocator), one stream
    synchronisation, and the returned arrays are views of that ONE block, which they keep alive (a caller that retains one of them for long retains all 111 MB of a
    640 x 640 pose: copy it out).  Six pageable `.double().cpu()` copies cost a 640 x 640 view more than its render (27.5 against 18.4 ms per pose, round 5).
    Round 6 tried the other order — transfer the float32 outputs (55 MB) and widen on the host with torch's CPU threads: 1.39 against 2.12 ms for the hand-over alone
    (profiles/r06_host_stacks.txt; numpy's single-threaded astype 11.6 ms), but inside the drivers the difference drowns in the thread pool's jitter (15.2-17.0 against
    15.6-16.4 ms per 640 x 640 pose, the 40-pose probabilistic call 19.8-23.2 against 19.7-20.8: profiles/r06_pose_drivers.txt) — not kept."""
    total = sum(int(np.prod(shape)) for _, shape in outputs)
    host = torch.empty(total, dtype=torch.float64, pin_memory=True)
    off = 0
    for t, shape in outputs:
        n = int(np.prod(shape))
        host[off:off + n].copy_(t.reshape(-1), non_blocking=True)
        off += n
    torch.cuda.current_stream(outputs[0][0].device).synchronize()
    arrays, off = [], 0
    for _, shape in outputs:
        n = int(np.prod(shape))
        arrays.append(host[off:off + n].numpy().reshape(shape))
        off += n
    return tuple(arrays)


@torch.no_grad()
def render_image_from_pose(radiance_field, estimator, poses, width, height, focal, near_plane, render_step_size, scale,
                           cone_angle, alpha_thre, downsample, device="cuda:0"):
    """Dataset.render_image_from_pose (habitat_to_data.py:304-411): all poses rendered in one batched call;
    returns host float64 arrays (images [P,h,w,3], depths [P,h,w], accs [P,h,w], sems [P,h,w,C])."""
    poses = np.asarray(poses)
    o, d, h, w = _pose_rays(poses, width, height, focal, scale, device)
    r = render_views(radiance_field, estimator, o, d, h * w, 1024, near_plane=near_plane, render_step_size=render_step_size,
                     render_bkgd=torch.zeros(3), cone_angle=cone_angle, alpha_thre=alpha_thre, image_hw=(h, w), n_split=None)
    P, C = poses.shape[0], radiance_field.num_semantic_classes
    return _host_stacks_f64([(r["rgb"], (P, h, w, 3)), (r["depth"], (P, h, w)), (r["acc"], (P, h, w)), (r["sem"], (P, h, w, C))])


@torch.no_grad()
def render_probablistic_image_from_pose(radiance_field, estimator, poses, width, height, focal, near_plane,
                                        render_step_size, scale, cone_angle, alpha_thre, downsample, device="cuda:0"):
    """Dataset.render_probablistic_image_from_pose (habitat_to_data.py:413-549) ->
    (images, images_var, depths, depths_var, accs, sems) host float64 arrays."""
    poses = np.asarray(poses)
    o, d, h, w = _pose_rays(poses, width, height, focal, scale, device)
    r = render_views(radiance_field, estimator, o, d, h * w, 1024, near_plane=near_plane, render_step_size=render_step_size,
                     render_bkgd=torch.zeros(3), cone_angle=cone_angle, alpha_thre=alpha_thre, probabilistic=True, image_hw=(h, w), n_split=None)
    P, C = poses.shape[0], radiance_field.num_semantic_classes
    return _host_stacks_f64([(r["rgb"], (P, h, w, 3)), (r["rgb_var"], (P, h, w, 3)), (r["depth"], (P, h, w)), (r["depth_var"], (P, h, w)), (r["acc"], (P, h, w)),
                             (r["sem"], (P, h, w, C))])


# ------------------------------------------------------------------ scorer (pipeline.py:666-798)
@torch.no_grad()
def score_view_terms(rgb_var, depth_var, acc, sem):
    """Per-view predictive-information terms on the device.  Inputs are member-major stacks of the probabilistic
    renders of M ensemble members for the same V views of P pixels: rgb_var [M,V,P,3], depth_var [M,V,P],
    acc [M,V,P], sem [M,V,P,C] (fp32, GPU).  Returns [V,4] float64: rgb, depth, semantic, occupancy (un-weighted)."""
    L.require_gpu(rgb_var, depth_var, acc, sem)
    M, V, P, C = sem.shape
    rv, dv, ac, sm = (L.contig(t, torch.float32) for t in (rgb_var, depth_var, acc, sem))
    terms = torch.empty(V, 4, dtype=torch.float64, device=sem.device)
    L.launch(L.load_library().mnf_score_views, L.ptr(rv), L.ptr(dv), L.ptr(ac), L.ptr(sm), M, V, P, C, L.ptr(terms))
    return terms


def shard_views(n_views: int, world: int, rank: int):
    """Contiguous view slice of `rank`: (lo, hi, per) with per = ceil(V / world) rows reserved per rank."""
    per = (n_views + world - 1) // world
    return min(rank * per, n_views), min((rank + 1) * per, n_views), per


def gather_view_terms(terms_local: torch.Tensor, n_views: int, group=None) -> torch.Tensor:
    """One all-gather of the per-rank [per,4] float64 term blocks (RCCL over xGMI on GPUs, gloo on CPU tensors);
    returns the [V,4] terms on every rank.  With no process group it is the identity."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) == 1:
        return terms_local[:n_views]
    world = dist.get_world_size(group)
    gathered = torch.empty(world * terms_local.shape[0], 4, dtype=terms_local.dtype, device=terms_local.device)
    all_gather_blocks(gathered, terms_local.contiguous(), group)
    return gathered[:n_views]


def all_gather_blocks(out: torch.Tensor, block: torch.Tensor, group=None) -> None:
    """`dist.all_gather_into_tensor(out, block)`: RCCL for device tensors; under the `gloo` backend (CPU test rigs, two processes sharing one GPU) device tensors
    are staged through the host, which is the only form gloo offers for them."""
    import torch.distributed as dist
    if block.is_cuda and dist.get_backend(group) == "gloo":
        host = torch.empty(out.shape, dtype=out.dtype)
        dist.all_gather_into_tensor(host, block.cpu(), group=group)
        out.copy_(host)
    else:
        dist.all_gather_into_tensor(out, block, group=group)


def trajectory_score(terms: torch.Tensor) -> torch.Tensor:
    """pipeline.py:775-781: rgb + depth + 3*sem + 2*occ, averaged over the views."""
    return (terms[:, 0] + terms[:, 1] + 3 * terms[:, 2] + 2 * terms[:, 3]).mean()


LAST_SCORE_TOTALS = []
_PROB_PLANES = (("rgb_var", (3,)), ("depth_var", ()), ("acc", ()), ("sem", (-1,)))      # name, trailing shape: what `score_view_terms` takes
_PLAIN_PLANES = (("rgb", (3,)), ("depth", ()), ("acc", ()))                             # `ensemble_view_terms`' (its sem is member 0's)


def _render_members(radiance_fields, estimators, o, d, P, planes, **opts):
    """The rays `o`, `d` (views of P pixels) rendered by every ensemble member with the scorers' fixed options and the caller's `opts`
    (near_plane, render_step_size, cone_angle, alpha_thre, probabilistic).  Returns (the member-major stacks [M,n,P,...] of `planes`, the
    members' render outputs)."""
    # every ensemble member renders the same rays: the members advance side by side as render jobs of one call (four jobs in
    # flight — the caller's stream + the library's three shared side streams — is the measured optimum for these small views,
    # profiles/r03_hw_queues.txt: two members are cut into two groups of views each, one member into four; rays stay in row-major
    # march order — the 8x8-block order of full images buys nothing on 64x64 sub-sampled views: profiles/r03_split_experiment.txt)
    M, n = len(radiance_fields), o.shape[0] // P
    outs = _render_jobs([(rf, est, o, d) for rf, est in zip(radiance_fields, estimators)], P, max_samples=1024, far_plane=1e10, render_bkgd=torch.zeros(3),
                        early_stop_eps=1e-4, n_split=max(1, 4 // M), **opts)
    return [torch.stack([r[k].reshape(n, P, *tail) for r in outs]) for k, tail in planes], outs


def _score_one_call(entry, workspace_bytes, radiance_fields, estimators, poses, width, height, focal, scale, device, **opts):
    """ONE C call `entry` (csrc/score.hip: mnf_score_poses, mnf_score_trajectory; `workspace_bytes` its size entry): poses -> the sub-sampled
    rays of every view -> renders by every ensemble member with `opts` (near_plane, render_step_size, cone_angle, alpha_thre, probabilistic)
    -> per-view terms [V,4] float64."""
    V, M = poses.shape[0], len(radiance_fields)
    c2w = torch.from_numpy(np.stack([pose_to_c2w(np.asarray(p, np.float64)) for p in poses]).astype(np.float32)[:, :3, :4].copy()).to(device)
    h, w = int(height * scale), int(width * scale)
    idx = torch.from_numpy(subsample_indices(width * height, h * w)).to(device)
    handles = (ctypes.c_void_p * M)(*[f._ensure_handle() for f in radiance_fields])
    grids = [_grid_args(e) for e in estimators]
    bins = (ctypes.c_void_p * M)(*[g.binaries.data_ptr() for g in grids])
    bits = (ctypes.c_void_p * M)(*[g.bits.data_ptr() for g in grids])
    ropts = _render_opts(max_samples=1024, far_plane=1e10, early_stop_eps=1e-4, rays_per_view=h * w, n_levels=grids[0].n_levels, **opts)   # row-major march order, as `score_views`
    nbytes = int(workspace_bytes(M, V, h * w, radiance_fields[0].num_semantic_classes))
    ws = _workspace(torch.device(device), nbytes)
    terms = torch.empty(V, 4, dtype=torch.float64, device=device)
    L.launch(entry, handles, bins, bits, M, *grids[0].res, grids[0].aabb, L.ptr(c2w), V, width,
             height, float(np.float32(focal)), L.ptr(idx), h * w, ctypes.byref(ropts), L.ptr(terms), L.ptr(ws), nbytes)
    return terms


def _check_view_planes(sem, V, planes, M=None):
    """The pixels per view P of the logits `sem`, [..., C] holding V views or (with `M`) [S,V,P,C], after checking that every (name, tensor, k)
    of `planes` holds V views (of each of M members) of P pixels of k floats; with `M` the first plane is [M,V,P,3] exactly."""
    C = int(sem.shape[-1])
    if M is None:
        if V == 0 or sem.numel() % (V * C):
            raise ValueError(f"sem of shape {tuple(sem.shape)} does not hold {V} views of {C}-class pixels")
        P = sem.numel() // (V * C)
    else:
        P = int(sem.shape[2])
    n = V * P * (1 if M is None else M)
    if any(t.numel() != n * k for _, t, k in planes) or (M is not None and tuple(planes[0][1].shape) != (M, V, P, 3)):
        raise ValueError(" / ".join(f"{name} {tuple(t.shape)}" for name, t, _ in planes) + " do not match "
                         + (f"{M} members of " if M is not None else "") + f"{V} views of {P} pixels")
    return P


@torch.no_grad()
def score_views(radiance_fields, estimators, poses, width, height, focal, near_plane, render_step_size, scale, cone_angle,
                alpha_thre, device="cuda:0", group=None):
    """Predictive information of candidate views, sharded over the ranks of `group` (pipeline.py:666-798 +
    SURVEY.md §8e): every rank renders its contiguous slice of `poses` with every ensemble member, reduces to
    per-view terms on the device, and one all-gather of [V,4] float64 gives every rank all terms.
    Returns (terms [V,4] float64 on device, score = mean_v(t0 + t1 + 3 t2 + 2 t3))."""
    import torch.distributed as dist
    poses = np.asarray(poses)
    V = poses.shape[0]
    world, rank = 1, 0
    if group is not False and dist.is_available() and dist.is_initialized():       # group=False: all views on this rank, no exchange
        world, rank = dist.get_world_size(group), dist.get_rank(group)
    lo, hi, per = shard_views(V, world, rank)
    terms_local = torch.zeros(per, 4, dtype=torch.float64, device=device)
    if hi > lo:
        o, d, h, w = _pose_rays(poses[lo:hi], width, height, focal, scale, device)
        stacks, outs = _render_members(radiance_fields, estimators, o, d, h * w, _PROB_PLANES, near_plane=near_plane, render_step_size=render_step_size,
                                       cone_angle=cone_angle, alpha_thre=alpha_thre, probabilistic=True)
        terms_local[:hi - lo] = score_view_terms(*stacks)
        LAST_SCORE_TOTALS[:] = [r["total"] for r in outs]       # per member: device int64 [kept, evaluated] samples of this rank's views (measurement aid)
    terms = terms_local[:V] if group is False else gather_view_terms(terms_local, V, group)
    return terms, trajectory_score(terms)


@torch.no_grad()
def score_poses(radiance_fields, estimators, poses, width, height, focal, near_plane, render_step_size, scale, cone_angle,
                alpha_thre, device="cuda:0"):
    """`score_views` on one rank as ONE C call (`mnf_score_poses`, csrc/score.hip): poses -> the sub-sampled rays of every
    view -> probabilistic renders by every ensemble member -> per-view terms.  Returns (terms [V,4] float64, score)."""
    lib = L.load_library()
    terms = _score_one_call(lib.mnf_score_poses, lib.mnf_score_poses_workspace_bytes, radiance_fields, estimators, np.asarray(poses), width, height, focal, scale, device,
                            near_plane=near_plane, render_step_size=render_step_size, cone_angle=cone_angle, alpha_thre=alpha_thre, probabilistic=True)
    return terms, trajectory_score(terms)


# ------------------------------------------------------------------ predictive-information maps (pipeline.py:727-774 kept per pixel)
SCORE_MAPS_MAX_MEMBERS, SCORE_MAPS_MAX_CLASSES = 64, 1024      # MNF_SCORE_MAPS_MAX_MEMBERS / _CLASSES (include/mi355nerf.h)


def _heat_range(heat_range):
    """(lo[4], hi[4]) -> two ctypes double[4] arrays, or (None, None)."""
    if heat_range is None:
        return None, None
    lo, hi = (np.asarray(x, np.float64).reshape(-1) for x in heat_range)
    if lo.size != 4 or hi.size != 4:
        raise ValueError("heat_range is (lo[4], hi[4]): one range per term (rgb, depth, semantic, occupancy)")
    if not (np.isfinite(lo).all() and np.isfinite(hi).all()) or (lo == hi).any():
        raise ValueError(f"heat_range needs finite lo != hi for every term (got lo {lo.tolist()}, hi {hi.tolist()})")
    return (ctypes.c_double * 4)(*lo), (ctypes.c_double * 4)(*hi)


def _view_maps_into(rv, dv, ac, sm, M, V, P, C, terms, maps, heat, lo, hi):
    """`mnf_score_view_maps` (csrc/infomap.hip) on contiguous fp32 stacks into `terms` [V,4] f64, `maps` [V,P,4] f64 and `heat` [V,P,4] u8
    (each a contiguous device tensor or None)."""
    lib = L.load_library()
    with torch.cuda.device(sm.device):
        nbytes = max(int(lib.mnf_score_view_maps_workspace_bytes(V, P, C)), 8)
        ws = _workspace((sm.device, "infomap"), nbytes)
        L.launch(lib.mnf_score_view_maps, L.ptr(rv), L.ptr(dv), L.ptr(ac), L.ptr(sm), M, V, P, C, L.ptr(terms), L.ptr(maps), L.ptr(heat), lo, hi, L.ptr(ws),
                 nbytes)


@torch.no_grad()
def view_information_maps(rgb_var, depth_var, acc, sem, *, maps=True, heat_range=None):
    """Where a candidate view carries predictive information: the four terms of `score_view_terms` kept per pixel, on the device
    (`mnf_score_view_maps`, csrc/infomap.hip).  Inputs as `score_view_terms` takes them: member-major stacks of the probabilistic renders
    of M ensemble members for the same V views of P pixels, rgb_var [M,V,P,3], depth_var [M,V,P], acc [M,V,P], sem [M,V,P,C] (fp32, GPU);
    up to 64 members and 1024 classes.  Returns (terms, maps, heat) and does not synchronise:
      terms [V,4] float64      the per-view means (rgb, depth, semantic, occupancy; un-weighted: `trajectory_score` weighs them);
      maps [V,P,4] float64     the terms of every pixel, or None with `maps=False`;
      heat [V,P,4] uint8       round(clip((x - lo_k) / (hi_k - lo_k) * 255, 0, 255)) (ties to even, NaN -> 0) for `heat_range` = (lo[4],
                               hi[4]), ready to index a colour table of the caller's; None without a range.
    A view's rows depend on that view's data only: a view scored alone or inside any batch gives the same bits."""
    if sem.dim() != 4 or rgb_var.dim() != 4 or rgb_var.shape[-1] != 3:
        raise ValueError(f"view_information_maps takes rgb_var [M,V,P,3] and sem [M,V,P,C] (got {tuple(rgb_var.shape)}, {tuple(sem.shape)})")
    M, V, P, C = (int(x) for x in sem.shape)
    _check_view_planes(sem, V, (("rgb_var", rgb_var, 3), ("depth_var", depth_var, 1), ("acc", acc, 1)), M)
    if min(M, P, C) < 1:
        raise ValueError(f"view_information_maps needs at least one member, pixel and class (got M = {M}, P = {P}, C = {C})")
    if M > SCORE_MAPS_MAX_MEMBERS or C > SCORE_MAPS_MAX_CLASSES:
        raise ValueError(f"{M} members of {C} classes are more than the supported {SCORE_MAPS_MAX_MEMBERS} members of {SCORE_MAPS_MAX_CLASSES} classes")
    lo, hi = _heat_range(heat_range)
    L.require_gpu(rgb_var, depth_var, acc, sem)
    rv, dv, ac, sm = (L.contig(t, torch.float32) for t in (rgb_var, depth_var, acc, sem))
    terms = torch.empty(V, 4, dtype=torch.float64, device=sem.device)
    out_maps = torch.empty(V, P, 4, dtype=torch.float64, device=sem.device) if maps else None
    heat = torch.empty(V, P, 4, dtype=torch.uint8, device=sem.device) if lo is not None else None
    _view_maps_into(rv, dv, ac, sm, M, V, P, C, terms, out_maps, heat, lo, hi)
    return terms, out_maps, heat


@torch.no_grad()
def score_view_maps(radiance_fields, estimators, poses, width, height, focal, near_plane, render_step_size, scale, cone_angle,
                    alpha_thre, device="cuda:0", *, heat_range=None, views_per_call=None):
    """`score_views` on one rank with the per-pixel maps kept: `poses` are rendered exactly as `score_views` renders them (the same render
    jobs with the same options), `views_per_call` poses at a time (None: all at once) so that the members' probabilistic planes exist for
    one group only (a 640 x 640 view holds 59 MB of them per member), and every group is reduced on the device (`view_information_maps`)
    into its slice of the outputs.  A view's render and its rows do not depend on the grouping, so neither do the bits.
    Returns a dict of device tensors: `terms` [V,4] float64, `score` = `trajectory_score(terms)`, `maps` [V,h,w,4] float64, and `heat`
    [V,h,w,4] uint8 for `heat_range` = (lo[4], hi[4]) (None without one)."""
    poses = np.asarray(poses)
    N, M = int(poses.shape[0]), len(radiance_fields)
    if N == 0:
        raise ValueError("score_view_maps needs at least one pose")
    lo, hi = _heat_range(heat_range)
    h, w = int(height * scale), int(width * scale)
    P, C = h * w, int(radiance_fields[0].num_semantic_classes)
    terms = torch.empty(N, 4, dtype=torch.float64, device=device)
    maps = torch.empty(N, P, 4, dtype=torch.float64, device=device)
    heat = torch.empty(N, P, 4, dtype=torch.uint8, device=device) if lo is not None else None
    per = N if views_per_call is None else max(1, int(views_per_call))
    for g0 in range(0, N, per):
        o, d, _, _ = _pose_rays(poses[g0:g0 + per], width, height, focal, scale, device)
        n = o.shape[0] // P
        stacks, _ = _render_members(radiance_fields, estimators, o, d, P, _PROB_PLANES, near_plane=near_plane, render_step_size=render_step_size,
                                    cone_angle=cone_angle, alpha_thre=alpha_thre, probabilistic=True)
        _view_maps_into(*(L.contig(t, torch.float32) for t in stacks), M, n, P, C, terms[g0:g0 + n], maps[g0:g0 + n],
                        heat[g0:g0 + n] if heat is not None else None, lo, hi)
    return dict(terms=terms, score=trajectory_score(terms), maps=maps.view(N, h, w, 4), heat=heat.view(N, h, w, 4) if heat is not None else None)


# ------------------------------------------------------------------ ensemble-disagreement scorer (pipeline.py:800-916)
ENSEMBLE_MAX_MEMBERS, ENSEMBLE_MAX_CLASSES = 64, 1024      # MNF_SCORE_ENSEMBLE_MAX_MEMBERS / _CLASSES (include/mi355nerf.h)


@torch.no_grad()
def ensemble_view_terms(rgb, depth, acc, sem):
    """The four clipped per-view rows of `trajector_uncertainty` (pipeline.py:861-882) on the device (`mnf_score_ensemble_views`,
    csrc/ensemble.hip).  Inputs are member-major stacks of the plain renders of M ensemble members for the same V views of P pixels:
    rgb [M,V,P,3], depth [M,V,P], acc [M,V,P] (member 0 is read), sem [V,P,C] (member 0's logits, as the reference keeps them) or
    [S,V,P,C] with 1 <= S <= M (the entropy is averaged over those members); fp32, GPU.  Returns [V,4] float64: 4000 x the
    across-member rgb variance and 50 x the depth variance, clipped to [0, 100]; mean clip(1 / (acc + 1e-4) - 1, 0, 10000); 50 x the
    softmax entropy, clipped to [0, 100]."""
    L.require_gpu(rgb, depth, acc, sem)
    if sem.dim() == 3:
        sem = sem[None]
    if sem.dim() != 4 or rgb.dim() != 4 or rgb.shape[-1] != 3:
        raise ValueError(f"ensemble_view_terms takes rgb [M,V,P,3] and sem [S,V,P,C] or [V,P,C] (got {tuple(rgb.shape)}, {tuple(sem.shape)})")
    S, V, P, C = (int(x) for x in sem.shape)
    M = int(rgb.shape[0])
    _check_view_planes(sem, V, (("rgb", rgb, 3), ("depth", depth, 1), ("acc", acc, 1)), M)
    lib = L.load_library()
    r, d, a, s = (L.contig(t, torch.float32) for t in (rgb, depth, acc, sem))
    terms = torch.empty(V, 4, dtype=torch.float64, device=sem.device)
    with torch.cuda.device(sem.device):
        nbytes = max(int(lib.mnf_score_ensemble_views_workspace_bytes(V, P, C)), 8)
        ws = _workspace((sem.device, "ensemble"), nbytes)
        L.launch(lib.mnf_score_ensemble_views, L.ptr(r), L.ptr(d), L.ptr(a), L.ptr(s), M, S, V, P, C, L.ptr(terms), L.ptr(ws), nbytes)
    return terms


def trajectory_view_indices(n_poses: int) -> np.ndarray:
    """The 40 poses of a trajectory that the scorers render (pipeline.py:687-689, :819-821): 20 evenly spread over all but the last
    20 poses, 20 over the last 20, truncated to integers."""
    a = np.linspace(0, n_poses - 20, 20)
    b = np.linspace(n_poses - 20, n_poses - 1, 20)
    return np.hstack((a, b)).astype(int)


def trajectory_uncertainty_from_terms(terms, step):
    """pipeline.py:883-896: per-view uncertainty = the sum of the four columns of `terms` [V,4]; `step == -1` averages the last 11
    views, any other step all of them.  Returns (uncertainty, max_idx); `max_idx` is `np.arange(V)` (the reference sorts its argsort)."""
    t = terms.detach().cpu().numpy() if isinstance(terms, torch.Tensor) else np.asarray(terms)
    per_view = t[:, 0] + t[:, 1] + t[:, 2] + t[:, 3]
    max_idx = np.sort(np.argsort(per_view))
    return (np.mean(per_view[-11:]) if step == -1 else np.mean(per_view[max_idx])), max_idx


@torch.no_grad()
def trajectory_uncertainty(radiance_fields, estimators, trajectory, step, width, height, focal, near_plane, render_step_size, cone_angle,
                           alpha_thre, scale=0.1, device="cuda:0", group=None, one_call=True):
    """`ActiveNeRFMapper.trajector_uncertainty` (pipeline.py:800-916): the 40 `trajectory_view_indices` poses of `trajectory` rendered by
    every ensemble member (plain render, black background, 1024 samples per round: `render_image_from_pose`), reduced to the four clipped
    rows on the device, ONE host copy of [V,4] doubles at the end.  `one_call=True` and no sharding: one C call (`mnf_score_trajectory`,
    csrc/score.hip); otherwise `_render_jobs` followed by `ensemble_view_terms`, the views sharded over the ranks of `group` exactly as
    `score_views` shards them (`group=False`: all views on this rank, no exchange).  All routes give the same bits.
    Returns (uncertainty, max_idx, rows): the first two as `trajectory_uncertainty_from_terms`, `rows` the [4,V] float64 host array
    that the reference appends to `trajector_uncertainty_list[step - 1]`."""
    import torch.distributed as dist
    trajectory = np.asarray(trajectory)
    poses = trajectory[trajectory_view_indices(len(trajectory))]
    V = poses.shape[0]
    world, rank = 1, 0
    if group is not False and dist.is_available() and dist.is_initialized():
        world, rank = dist.get_world_size(group), dist.get_rank(group)
    if one_call and world == 1:
        lib = L.load_library()
        terms = _score_one_call(lib.mnf_score_trajectory, lib.mnf_score_trajectory_workspace_bytes, radiance_fields, estimators, poses, width, height, focal, scale,
                                device, near_plane=near_plane, render_step_size=render_step_size, cone_angle=cone_angle, alpha_thre=alpha_thre, probabilistic=False)
    else:
        lo, hi, per = shard_views(V, world, rank)
        terms_local = torch.zeros(per, 4, dtype=torch.float64, device=device)
        if hi > lo:
            o, d, h, w = _pose_rays(poses[lo:hi], width, height, focal, scale, device)
            stacks, outs = _render_members(radiance_fields, estimators, o, d, h * w, _PLAIN_PLANES, near_plane=near_plane,
                                           render_step_size=render_step_size, cone_angle=cone_angle, alpha_thre=alpha_thre, probabilistic=False)
            terms_local[:hi - lo] = ensemble_view_terms(*stacks, outs[0]["sem"].reshape(hi - lo, h * w, -1))
        terms = terms_local[:V] if world == 1 else gather_view_terms(terms_local, V, group)
    rows = np.ascontiguousarray(terms.cpu().numpy().T)            # the one device-to-host copy
    uncertainty, max_idx = trajectory_uncertainty_from_terms(rows.T, step)
    return uncertainty, max_idx, rows


# ------------------------------------------------------------------ held-out view evaluation (pipeline.py:550-613, :650-656, :1011)
EVAL_COLUMNS = ("rgb_mse", "psnr", "depth_mse", "sem_ce", "sem_acc", "n_valid", "n_invalid", "reserved")     # columns of mnf_eval_views' metrics rows


def miou_from_confusion(confusion) -> float:
    """Mean intersection over union of a [C,C] confusion matrix (rows: ground-truth class, columns: predicted class): the mean of
    TP / (TP + FP + FN) over the classes that occur in the ground truth or in the prediction; a class absent from both does not enter
    the mean.  NaN for an all-zero matrix.  Pure numpy / torch, no GPU."""
    m = confusion.detach().cpu().numpy() if isinstance(confusion, torch.Tensor) else np.asarray(confusion)
    m = m.astype(np.float64)
    tp = np.diag(m)
    union = m.sum(0) + m.sum(1) - tp            # TP + FP + FN
    present = union > 0
    if not present.any():
        return float("nan")
    return float(np.mean(tp[present] / union[present]))


def _eval_index_tensor(idx, device, limit, what):
    """int64 device tensor of `idx`; a host list / array / tensor is range-checked here (a device tensor is the caller's word: checking
    it would take a synchronisation)."""
    if isinstance(idx, torch.Tensor) and idx.is_cuda:
        return L.contig(idx.reshape(-1), torch.int64)
    host = np.asarray(idx.cpu() if isinstance(idx, torch.Tensor) else idx).astype(np.int64).reshape(-1)
    if host.size and (host.min() < 0 or host.max() >= limit):
        raise IndexError(f"{what} out of range [0, {limit})")
    return torch.from_numpy(host).to(device)


@torch.no_grad()
def eval_metrics(rgb, depth, sem, dataset, image_ids, pix_idx=None, confusion=True, labels=False):
    """Error metrics of finished renders against the ground truth a `Dataset` holds (`mnf_eval_views`, csrc/eval.hip): rgb [V,P,3],
    depth [V,P] / [V,P,1], sem [V,P,C] (or their [V,H,W,...] forms) for the images `image_ids` [V]; pixel p of a view is pixel
    `pix_idx[p]` of its image (None: pixel p, row-major).  The ground truth is read from `dataset.images / depths / semantics` as they
    are stored, `packed=True` or not; no fp32 ground-truth image is made.  Returns a dict of device tensors and does not synchronise:
    `metrics` [V,8] float64 (columns: EVAL_COLUMNS), `confusion` [C,C] int64 summed over the V views (None unless `confusion`),
    `pred_labels` [V,P] uint8 (None unless `labels`)."""
    lib = L.load_library()
    L.require_gpu(rgb, depth, sem, dataset.images, dataset.depths, dataset.semantics)
    dev = sem.device
    C = int(sem.shape[-1])
    ids = _eval_index_tensor(image_ids, dev, len(dataset), "image_ids")
    V = int(ids.shape[0])
    ppi = int(dataset.height) * int(dataset.width)
    P = _check_view_planes(sem, V, (("rgb", rgb, 3), ("depth", depth, 1)))
    pix = None
    if pix_idx is not None:
        pix = _eval_index_tensor(pix_idx, dev, ppi, "pix_idx")
        if int(pix.shape[0]) != P:
            raise ValueError(f"pix_idx has {int(pix.shape[0])} entries for views of {P} pixels")
    elif P > ppi:
        raise ValueError(f"views of {P} pixels against images of {ppi} pixels need a pix_idx")
    if labels and C > 256:
        raise ValueError("pred_labels are uint8: labels=True needs at most 256 classes")
    if dataset.depths.dtype not in (torch.float32, torch.float16) or dataset.semantics.dtype not in (torch.int64, torch.uint8) \
            or dataset.images.dtype != torch.uint8:
        raise TypeError("eval_metrics reads u8 images, f32 / f16 depths and i64 / u8 labels")
    r, d, s = (L.contig(t, torch.float32) for t in (rgb, depth, sem))
    gi, gd, gs = dataset.images.contiguous(), dataset.depths.contiguous(), dataset.semantics.contiguous()
    metrics = torch.empty(V, 8, dtype=torch.float64, device=dev)
    conf = torch.empty(C, C, dtype=torch.int64, device=dev) if confusion else None
    pred = torch.empty(V, P, dtype=torch.uint8, device=dev) if labels else None
    with torch.cuda.device(dev):
        nbytes = int(lib.mnf_eval_views_workspace_bytes(V, P, C))
        ws = _workspace((dev, "eval"), max(nbytes, 8))
        L.launch(lib.mnf_eval_views, L.ptr(r), L.ptr(d), L.ptr(s), V, P, C, L.ptr(gi), L.ptr(gd), int(gd.dtype == torch.float16), L.ptr(gs),
                 int(gs.dtype == torch.uint8), ppi, L.ptr(ids), L.ptr(pix), L.ptr(metrics), L.ptr(conf), L.ptr(pred), L.ptr(ws), max(nbytes, 8))
    return dict(metrics=metrics, confusion=conf, pred_labels=pred)


# structural similarity (Wang et al. 2004) over the valid windows: skimage's gaussian_weights=True form, mip-NeRF's compute_ssim
SSIM_WINDOW, SSIM_SIGMA = 11, 1.5      # MNF_SSIM_WINDOW / MNF_SSIM_SIGMA (include/mi355nerf.h): fixed
SSIM_K1, SSIM_K2 = 0.01, 0.03
SSIM_MAX_CHANNELS = 4                  # MNF_SSIM_MAX_CHANNELS


def _ssim_into(pred, target, target_u8, ids, ppi, V, H, W, K, data_range, ssim, maps, k1=SSIM_K1, k2=SSIM_K2):
    """`mnf_ssim_views` (csrc/ssim.hip) on contiguous device tensors: `pred` [V,H,W,K] f32 against `target` (f32, same shape) or against
    `target_u8` (dataset storage, view v = image `ids[v]`) into `ssim` [V] f64 and `maps` [V,H-10,W-10] f64 or None."""
    lib = L.load_library()
    with torch.cuda.device(pred.device):
        nbytes = max(int(lib.mnf_ssim_views_workspace_bytes(V, H, W, K)), 8)
        ws = _workspace((pred.device, "ssim"), nbytes)
        L.launch(lib.mnf_ssim_views, L.ptr(pred), L.ptr(target), L.ptr(target_u8), L.ptr(ids), ppi, V, H, W, K, float(data_range), float(k1), float(k2),
                 L.ptr(ssim), L.ptr(maps), L.ptr(ws), nbytes)


def _ssim_outputs(V, H, W, maps, device):
    ssim = torch.empty(V, dtype=torch.float64, device=device)
    return ssim, (torch.empty(V, H - SSIM_WINDOW + 1, W - SSIM_WINDOW + 1, dtype=torch.float64, device=device) if maps else None)


@torch.no_grad()
def ssim_views(pred, target, *, data_range=1.0, maps=False):
    """Structural similarity of V views against V targets on the device (`mnf_ssim_views`, csrc/ssim.hip): what
    `skimage.metrics.structural_similarity(gaussian_weights=True, sigma=1.5, use_sample_covariance=False, data_range=data_range,
    channel_axis=-1)` returns after its border crop — the 11 x 11 Gaussian window over the valid windows only, in float64 from the fp32
    values.  `pred` and `target` are [V,H,W,K] fp32 GPU tensors, K <= 4; a [V,H,W] plane is K = 1.  Not only rgb: depth against depth with
    `data_range` = the depth span, or one ensemble member's render against another's.
    Returns dict(ssim=[V] float64, maps=[V,H-10,W-10] float64 | None) as device tensors (a map is the mean of the channels' SSIM at every
    window centre) and does not synchronise.  A view's bits do not depend on the other views of the call."""
    if pred.shape != target.shape or pred.dim() not in (3, 4):
        raise ValueError(f"ssim_views takes pred and target of one shape [V,H,W,K] or [V,H,W] (got {tuple(pred.shape)}, {tuple(target.shape)})")
    V, H, W = (int(x) for x in pred.shape[:3])
    K = int(pred.shape[3]) if pred.dim() == 4 else 1
    if not 1 <= K <= SSIM_MAX_CHANNELS:
        raise ValueError(f"ssim_views takes 1 to {SSIM_MAX_CHANNELS} channels (got {K})")
    if not (np.isfinite(data_range) and data_range > 0):
        raise ValueError(f"data_range must be finite and positive (got {data_range})")
    if H < SSIM_WINDOW or W < SSIM_WINDOW:
        raise ValueError(f"SSIM's {SSIM_WINDOW} x {SSIM_WINDOW} window needs images of at least that size (got {H} x {W})")
    L.require_gpu(pred, target)
    ssim, out_maps = _ssim_outputs(V, H, W, maps, pred.device)
    _ssim_into(L.contig(pred, torch.float32), L.contig(target, torch.float32), None, None, 0, V, H, W, K, data_range, ssim, out_maps)
    return dict(ssim=ssim, maps=out_maps)


@torch.no_grad()
def ssim_metrics(rgb, dataset, image_ids, *, maps=False):
    """`ssim_views` of finished rgb renders against the images a `Dataset` holds: rgb [V,H,W,3] or [V,P,3] (P = the dataset's height x
    width) for the images `image_ids` [V].  `dataset.images` is read as it is stored (u8, (float)u8 / 255.0f per channel: the pixels
    `Dataset.__getitem__` hands out); no fp32 ground-truth image is made.  data_range is 1.  Returns what `ssim_views` returns."""
    L.require_gpu(rgb, dataset.images)
    if dataset.images.dtype != torch.uint8:
        raise TypeError("ssim_metrics reads u8 images")
    H, W = int(dataset.height), int(dataset.width)
    ids = _eval_index_tensor(image_ids, rgb.device, len(dataset), "image_ids")
    V = int(ids.shape[0])
    if rgb.dim() not in (3, 4) or int(rgb.shape[0]) != V or int(rgb.shape[-1]) != 3 or rgb.numel() != V * H * W * 3:
        raise ValueError(f"ssim_metrics takes rgb [V,H,W,3] or [V,H*W,3] of {V} views of {H} x {W} pixels (got {tuple(rgb.shape)})")
    if H < SSIM_WINDOW or W < SSIM_WINDOW:
        raise ValueError(f"SSIM's {SSIM_WINDOW} x {SSIM_WINDOW} window needs images of at least that size (got {H} x {W})")
    ssim, out_maps = _ssim_outputs(V, H, W, maps, rgb.device)
    _ssim_into(L.contig(rgb, torch.float32), None, dataset.images.contiguous(), ids, H * W, V, H, W, 3, 1.0, ssim, out_maps)
    return dict(ssim=ssim, maps=out_maps)


@torch.no_grad()
def evaluate_views(radiance_field, estimator, dataset, indices, *, near_plane, render_step_size, cone_angle, alpha_thre, max_samples=1024,
                   render_bkgd=None, views_per_call=4, return_images=False, labels=False, ssim=False):
    """The evaluation block of `nerf_training` (pipeline.py:550-613) as one call: the held-out images `indices` of `dataset` are rendered
    `views_per_call` at a time — one batched `mnf_generate_rays` (all pixels, row-major: the evaluation branch of `Dataset.fetch_data`),
    one batched test render (a view's result is that of `render_image_with_occgrid_test` on `dataset[i]["rays"]`, bit for bit, whatever
    the grouping) and one `mnf_eval_views` per group — and ONE device-to-host copy at the end brings the metrics and the confusion matrix.
    `render_bkgd=None` is white, what `Dataset.preprocess` hands out when not training.
    Returns a dict: per-view float64 arrays `rgb_mse`, `psnr`, `depth_mse`, `sem_ce`, `sem_acc`; `confusion` int64 [C,C] over all views
    with `pixel_accuracy` and `miou` (`miou_from_confusion`); `mean` = {"psnr", "depth_mse", "sem_ce"}, the three numbers
    pipeline.py:650-656 prints.  Raises ValueError when a view has labels outside [0, C) (so does torch's cross_entropy).
    `return_images=True` adds the device tensors `rgb` [N,H,W,3], `acc` [N,H,W,1], `depth` [N,H,W,1], `sem` [N,H,W,C], and
    `pred_labels` [N,H,W] uint8 with `labels=True` (the argmax image of pipeline.py:1011).
    `ssim=True` adds `ssim`, the per-view float64 structural similarity of the rgb render against the stored image (`ssim_metrics`, on
    the device, in the same single copy), and `mean["ssim"]`."""
    lib = L.load_library()
    idx = [int(i) for i in (indices.tolist() if hasattr(indices, "tolist") else indices)]
    if not idx:
        raise ValueError("evaluate_views needs at least one image index")
    if min(idx) < 0 or max(idx) >= len(dataset):
        raise IndexError(f"image index out of range [0, {len(dataset)})")
    H, W = int(dataset.height), int(dataset.width)
    P, C = H * W, int(radiance_field.num_semantic_classes)
    dev = dataset.images.device
    L.require_gpu(dataset.images, dataset.camtoworlds)
    bkgd = torch.ones(3) if render_bkgd is None else render_bkgd.detach().cpu()      # a host tensor: the render options take host floats
    per = max(1, int(views_per_call))
    rows, conf, imgs, sims = [], None, dict(rgb=[], acc=[], depth=[], sem=[], pred_labels=[]), []
    for g0 in range(0, len(idx), per):
        ids = torch.tensor(idx[g0:g0 + per], dtype=torch.int64, device=dev)
        V = int(ids.shape[0])
        c2w = dataset.camtoworlds[ids][:, :3, :4].contiguous()
        o = torch.empty(V * P, 3, device=dev)
        d = torch.empty(V * P, 3, device=dev)
        L.launch(lib.mnf_generate_rays, L.ptr(c2w), V, W, H, dataset._focal, None, P, L.ptr(o), L.ptr(d))
        r = _render_jobs([(radiance_field, estimator, o, d)], P, max_samples=max_samples, near_plane=near_plane, far_plane=1e10, render_step_size=render_step_size,
                         render_bkgd=bkgd, cone_angle=cone_angle, alpha_thre=alpha_thre, early_stop_eps=1e-4, probabilistic=False, image_hw=(H, W), n_split=None)[0]
        m = eval_metrics(r["rgb"], r["depth"], r["sem"], dataset, ids, None, confusion=True, labels=labels and return_images)
        rows.append(m["metrics"])
        conf = m["confusion"] if conf is None else conf + m["confusion"]
        if ssim:
            sims.append(ssim_metrics(r["rgb"].view(V, H, W, 3), dataset, ids)["ssim"])
        if return_images:
            for k in ("rgb", "acc", "depth", "sem"):
                imgs[k].append(r[k].view(V, H, W, -1))
            if labels:
                imgs["pred_labels"].append(m["pred_labels"].view(V, H, W))
    n = len(idx)
    # the one device-to-host copy: the metric rows and the matrix (its int64 bits carried as float64 words) in one block
    host = torch.cat([torch.cat(rows).reshape(-1), conf.view(torch.float64).reshape(-1)] + sims).cpu()
    met = host[:n * 8].numpy().reshape(n, 8)
    confusion = host[n * 8:n * 8 + C * C].view(torch.int64).numpy().reshape(C, C).copy()
    if (met[:, 6] > 0).any():
        bad = [idx[k] for k in np.nonzero(met[:, 6] > 0)[0]]
        raise ValueError(f"ground-truth labels outside [0, {C}) in image(s) {bad}: {int(met[:, 6].sum())} pixels")
    out = {name: met[:, k].copy() for k, name in enumerate(EVAL_COLUMNS[:5])}
    total = confusion.sum()
    out["confusion"] = confusion
    out["pixel_accuracy"] = float(np.trace(confusion) / total) if total else float("nan")
    out["miou"] = miou_from_confusion(confusion)
    out["mean"] = {"psnr": float(np.mean(out["psnr"])), "depth_mse": float(np.mean(out["depth_mse"])), "sem_ce": float(np.mean(out["sem_ce"]))}
    if ssim:
        out["ssim"] = host[n * 8 + C * C:].numpy().copy()
        out["mean"]["ssim"] = float(np.mean(out["ssim"]))
    if return_images:
        for k in ("rgb", "acc", "depth", "sem") + (("pred_labels",) if labels else ()):
            out[k] = torch.cat(imgs[k])
    return out


# ------------------------------------------------------------------ 8-bit frames (pipeline.py:918-1023, vis_nerf_habitat.py:142-179)
FRAME_DEPTH_PIPELINE = (25.0, 1.0, 255.0, 1.0)      # (mul, div, clip_hi, gain): np.clip(dep * 25, 0, 255), pipeline.py:1003
FRAME_DEPTH_VIEWER = (1.0, 10.0, 1.0, 255.0)        # np.clip(depth / 10, 0, 1) * 255, vis_nerf_habitat.py:142-179
_FRAME_PLANES = (("rgb", 3), ("depth", 1), ("occ", 1), ("sem", 3), ("labels", 1))      # name, bytes per pixel


def _frame_palette(palette, device, n_classes):
    pal = palette if isinstance(palette, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(palette))
    if pal.dtype != torch.uint8 or pal.dim() != 2 or pal.shape[1] != 3:
        raise TypeError(f"palette must be a [K,3] uint8 array or tensor (got {tuple(pal.shape)} {pal.dtype})")
    if pal.shape[0] < n_classes:
        raise ValueError(f"palette has {pal.shape[0]} colours for {n_classes} classes")
    return pal.to(device).contiguous()


def _frame_args(depth_map, channel_order, labels, n_classes):
    if channel_order not in ("bgr", "rgb"):
        raise ValueError(f"channel_order must be 'bgr' or 'rgb' (got {channel_order!r})")
    if labels and n_classes > 256:
        raise ValueError("the label plane is uint8: labels=True needs at most 256 classes")
    dm = tuple(float(x) for x in depth_map)
    if len(dm) != 4:
        raise ValueError("depth_map is (mul, div, clip_hi, gain): FRAME_DEPTH_PIPELINE, FRAME_DEPTH_VIEWER or four numbers of the caller's")
    return dm, int(channel_order == "bgr")


def _frames_into(rgb, depth, acc, sem, pal, dm, bgr, out):
    """`mnf_frames_views` (csrc/frames.hip) on V views of P pixels into the contiguous uint8 tensors of `out` (keys of _FRAME_PLANES; no
    "labels" key: no label plane)."""
    V, C = int(sem.shape[0]), int(sem.shape[-1])
    P = _check_view_planes(sem, V, (("rgb", rgb, 3), ("depth", depth, 1), ("acc", acc, 1)))
    for name, k in _FRAME_PLANES:
        if name in out and (out[name].dtype != torch.uint8 or out[name].numel() != V * P * k or not out[name].is_contiguous()):
            raise ValueError(f"output plane {name} does not hold {V} x {P} x {k} contiguous bytes")
    r, d, a, s = (L.contig(t, torch.float32) for t in (rgb, depth, acc, sem))
    L.launch(L.load_library().mnf_frames_views, L.ptr(r), L.ptr(d), L.ptr(a), L.ptr(s), V, P, C, L.ptr(pal), int(pal.shape[0]), *dm, bgr,
             L.ptr(out["rgb"]), L.ptr(out["depth"]), L.ptr(out["occ"]), L.ptr(out["sem"]), L.ptr(out.get("labels")))


@torch.no_grad()
def frames_from_renders(rgb, depth, acc, sem, palette, *, depth_map=FRAME_DEPTH_PIPELINE, channel_order="bgr", labels=False):
    """The 8-bit frames of finished renders (`mnf_frames_views`, csrc/frames.hip), as `ActiveNeRFMapper.render` writes them with `cv2.imwrite`
    (pipeline.py:976-1023): rgb [V,P,3], depth and acc [V,P] / [V,P,1], sem [V,P,C] device planes (or their [V,H,W,...] forms), `palette` any
    [K,3] uint8 RGB array or tensor with K >= C (the reference's is habitat_sim's `d3_40_colors_rgb`).  Returns a dict of device uint8
    tensors with the inputs' leading shape and does not synchronise: `rgb` [...,3] = round(x * 255) in float32, `depth` = round(clip(d * mul
    / div, 0, clip_hi) * gain) in float64 with `depth_map` = (mul, div, clip_hi, gain) (FRAME_DEPTH_PIPELINE: clip(dep * 25, 0, 255);
    FRAME_DEPTH_VIEWER: clip(depth / 10, 0, 1) * 255), `occ` = round(acc * 255), `sem` [...,3] = palette[argmax], and with `labels=True`
    `labels` = the argmax itself (C <= 256).  Rounding is to nearest, ties to even, after clamping to [0, 255]; a NaN gives 0.
    `channel_order="bgr"` stores the two colour planes as `cv2.imwrite` takes them, "rgb" as they are."""
    L.require_gpu(rgb, depth, acc, sem)
    C = int(sem.shape[-1])
    dm, bgr = _frame_args(depth_map, channel_order, labels, C)
    pal = _frame_palette(palette, sem.device, C)
    lead = tuple(sem.shape[:-1])
    out = {name: torch.empty(*lead, *((k,) if k == 3 else ()), dtype=torch.uint8, device=sem.device)
           for name, k in _FRAME_PLANES if name != "labels" or labels}
    _frames_into(rgb, depth, acc, sem, pal, dm, bgr, out)
    return out


@torch.no_grad()
def render_frames(radiance_field, estimator, poses, width, height, focal, near_plane, render_step_size, scale, cone_angle, alpha_thre, palette, *,
                  depth_map=FRAME_DEPTH_PIPELINE, channel_order="bgr", labels=False, views_per_call=4, max_samples=1024, to_host=True, device="cuda:0"):
    """`ActiveNeRFMapper.render`'s predicted frames (pipeline.py:955-1023) as one call: `poses` are rendered exactly as `render_image_from_pose`
    renders them (the same rays, options and black background), `views_per_call` at a time so that float planes exist for one group only, and
    every group is converted on the device (`frames_from_renders`) into its slice of ONE uint8 block: 8 bytes per pixel (9 with `labels`)
    instead of the 272 of the float64 stacks.  A view's render does not depend on the grouping, so neither do the bytes.
    `to_host=True`: one device-to-host copy into one pinned block and one synchronisation at the end; the returned numpy arrays `rgb`
    [P,h,w,3], `depth` [P,h,w], `occ` [P,h,w], `sem` [P,h,w,3] (and `labels` [P,h,w]) are views of that ONE block, which they keep alive: a
    caller that retains one of them for long retains all of them (copy it out).  `to_host=False`: the device tensors, no synchronisation."""
    poses = np.asarray(poses)
    N, C = int(poses.shape[0]), int(radiance_field.num_semantic_classes)
    if N == 0:
        raise ValueError("render_frames needs at least one pose")
    dm, bgr = _frame_args(depth_map, channel_order, labels, C)
    pal = _frame_palette(palette, device, C)
    h, w = int(height * scale), int(width * scale)
    P = h * w
    planes = [(name, k) for name, k in _FRAME_PLANES if name != "labels" or labels]
    block = torch.empty(N * P * sum(k for _, k in planes), dtype=torch.uint8, device=device)
    flat, off = {}, 0
    for name, k in planes:
        flat[name] = block[off:off + N * P * k].view(N, P * k)
        off += N * P * k
    per = max(1, int(views_per_call))
    for g0 in range(0, N, per):
        o, d, _, _ = _pose_rays(poses[g0:g0 + per], width, height, focal, scale, device)
        V = o.shape[0] // P
        r = render_views(radiance_field, estimator, o, d, P, max_samples, near_plane=near_plane, render_step_size=render_step_size,
                         render_bkgd=torch.zeros(3), cone_angle=cone_angle, alpha_thre=alpha_thre, image_hw=(h, w), n_split=None)
        _frames_into(r["rgb"].view(V, P, 3), r["depth"].view(V, P), r["acc"].view(V, P), r["sem"].view(V, P, C), pal, dm, bgr,
                     {name: flat[name][g0:g0 + V] for name, _ in planes})
    if to_host:
        host = torch.empty(block.numel(), dtype=torch.uint8, pin_memory=True)
        host.copy_(block, non_blocking=True)
        torch.cuda.current_stream(block.device).synchronize()
        whole = host.numpy()
    out, off = {}, 0
    for name, k in planes:
        shape = (N, h, w) + ((3,) if k == 3 else ())
        out[name] = (whole if to_host else block)[off:off + N * P * k].reshape(shape)
        off += N * P * k
    return out
