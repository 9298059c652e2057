"""Relocalisation of captures against the frozen map: batched pose refinement on the device (`mnf_pose_refine`, csrc/localize.hip).

The paper's list starts with state estimation; the reference gets exact poses from Habitat, a robot with odometry does not.  `PoseRefiner` corrects the
camera poses of B stored captures before they are trained on: one 6-vector `xi[b] = (rotvec, trans)` per view relative to its initial pose, optimised with
Adam against the field with its parameters frozen — what INTEGRATION.md §A's loop (`transform_rays` -> `fused_train_render_rays` -> loss -> `backward()` ->
`torch.optim.Adam`) does for one view and one iteration per host round, here for all views in one forward and one backward per iteration and a whole run
of iterations per C call, with no host synchronisation inside the run.

    ref = PoseRefiner(field, estimator, dataset, image_ids, **RENDER_KW)      # initial poses: the dataset's own
    ref.step(50)                                                              # enqueues 50 iterations, returns nothing
    out = ref.result()                                                        # ONE host copy
    dataset.set_camtoworlds(image_ids, out["c2w"])

Limits: the sample set is a constant of each render (no gradient through the sample positions, as on both torch routes); no hand-over to the call-by-call
route (at most four occupancy levels; a ray past the sampler's scratch row stalls the iteration and shows as status bit 2); one GPU."""
import ctypes

import numpy as np
import torch

from . import _lib as L
from . import render as RD

WS_RAYS_O, WS_RAYS_D, WS_PIX, WS_RGB, WS_ACC, WS_DEPTH, WS_SEM, WS_G_RAYS_O, WS_G_RAYS_D, WS_GRAD, WS_ROT, WS_KEPT = range(12)      # MNF_POSE_WS_*


def rodrigues(rotvec):
    """R [..,3,3] float64 of axis-angle vectors [..,3] on the host, with `transform_rays`' branches (series below t^2 = 1e-6)."""
    k = np.asarray(rotvec, np.float64)
    t2 = (k * k).sum(-1)
    small = t2 < 1e-6
    t = np.sqrt(np.where(small, 1.0, t2))
    a = np.where(small, 1.0 - t2 / 6.0 + t2 * t2 / 120.0, np.sin(t) / t)
    b = np.where(small, 0.5 - t2 / 24.0 + t2 * t2 / 720.0, (1.0 - np.cos(t)) / np.where(small, 1.0, t2))
    K = np.zeros(k.shape[:-1] + (3, 3))
    K[..., 0, 1], K[..., 0, 2], K[..., 1, 0], K[..., 1, 2], K[..., 2, 0], K[..., 2, 1] = -k[..., 2], k[..., 1], k[..., 2], -k[..., 0], -k[..., 1], k[..., 0]
    return np.eye(3) + a[..., None, None] * K + b[..., None, None] * (K @ K)


def compose_c2w(c2w0, xi):
    """[B,4,4] float64: the initial poses [B,3|4,4] under the corrections xi [B,6]: [R(rotvec) R0 | c + trans]."""
    c2w0, xi = np.asarray(c2w0, np.float64), np.asarray(xi, np.float64)
    out = np.tile(np.eye(4), (c2w0.shape[0], 1, 1))
    out[:, :3, :3] = rodrigues(xi[:, :3]) @ c2w0[:, :3, :3]
    out[:, :3, 3] = c2w0[:, :3, 3] + xi[:, 3:]
    return out


class PoseRefiner:
    """Holds the corrections `xi`, Adam's moments and the workspace of a refinement of `image_ids` (views stored in `dataset`) against `radiance_field`.

      c2w0            initial poses [B,3|4,4] (host or device); None: the dataset's stored poses of those images
      rays_per_view   pixels per view and iteration, drawn anew every iteration on the device (Philox, key `seed`) unless `pix_idx` [B,n] (flat ids
                      y * W + x) fixes them
      lr_rot, lr_trans, betas, eps   Adam on the six numbers of every view;  weights: of the rgb / depth / semantic terms (pipeline.py:511)
      render_kw       the train render's options, as `fused_train_render_rays` takes them (near_plane, far_plane, render_step_size, cone_angle, alpha_thre,
                      early_stop_eps, render_bkgd); the render never jitters

    Sample bounds are the field's (`render.reserve_sample_bounds`); after a bounds bit in `result()["status"]` reserve more and step again — the refiner
    does not loop on its own, the views stalled meanwhile.  The field's parameters are read, never written, whatever their `requires_grad`."""

    def __init__(self, radiance_field, estimator, dataset, image_ids, c2w0=None, *, rays_per_view=1024, lr_rot=1e-3, lr_trans=2e-3, weights=(10.0, 0.2, 0.5),
                 seed=0, pix_idx=None, betas=(0.9, 0.999), eps=1e-15, **render_kw):
        if estimator.levels > 4:
            raise L.MnfError("PoseRefiner: more than four occupancy levels (no hand-over to the call-by-call route happens inside the refiner)")
        self.field, self.estimator, self.dataset = radiance_field, estimator, dataset
        dev = radiance_field.mlp_base.params.device
        L.require_gpu(radiance_field.mlp_base.params, dataset.images, dataset.depths, dataset.semantics)
        ids = torch.as_tensor(image_ids).reshape(-1).to(torch.int64).cpu()
        if ids.numel() == 0 or int(ids.min()) < 0 or int(ids.max()) >= dataset.size:
            raise ValueError(f"PoseRefiner: image_ids must be a non-empty list of ids in [0, {dataset.size})")
        self.B, self.n = int(ids.numel()), int(rays_per_view)
        if self.n <= 0:
            raise ValueError("PoseRefiner: rays_per_view must be positive")
        self.image_ids = ids.to(dev)
        c2w = dataset.camtoworlds[self.image_ids] if c2w0 is None else torch.as_tensor(c2w0)
        if c2w.dim() != 3 or c2w.shape[0] != self.B or c2w.shape[1] not in (3, 4) or c2w.shape[2] != 4:
            raise ValueError(f"PoseRefiner: c2w0 must be [{self.B},3|4,4] (got {tuple(c2w.shape)})")
        self.c2w0 = c2w[:, :3, :4].to(device=dev, dtype=torch.float32).contiguous()
        self._c2w0_host = None      # (read in result(): its one host copy carries it)
        self.H, self.W = int(dataset.height), int(dataset.width)
        self.pix_idx = None
        if pix_idx is not None:
            p = torch.as_tensor(pix_idx).to(torch.int64)
            if tuple(p.shape) != (self.B, self.n) or int(p.min()) < 0 or int(p.max()) >= self.H * self.W:
                raise ValueError(f"PoseRefiner: pix_idx must be [{self.B},{self.n}] flat pixel ids in [0, {self.H * self.W})")
            self.pix_idx = p.to(dev).contiguous()
        self.pose = L.PoseOpts()
        self.pose.w_rgb, self.pose.w_dep, self.pose.w_sem = (float(w) for w in weights)
        self.pose.lr_rot, self.pose.lr_trans, self.pose.beta1, self.pose.beta2, self.pose.eps = float(lr_rot), float(lr_trans), float(betas[0]), float(betas[1]), float(eps)
        self.pose.seed = int(seed)
        self.render_kw = dict(near_plane=0.0, far_plane=1e10, render_step_size=1e-3, cone_angle=0.0, alpha_thre=0.0, early_stop_eps=1e-4)
        self.render_bkgd = render_kw.pop("render_bkgd", None)
        unknown = set(render_kw) - set(self.render_kw)
        if unknown:
            raise TypeError(f"PoseRefiner: unknown render options {sorted(unknown)}")
        self.render_kw.update(render_kw)
        self.xi = torch.zeros(self.B, 6, dtype=torch.float64, device=dev)
        self.adam_m, self.adam_v = torch.zeros_like(self.xi), torch.zeros_like(self.xi)
        self.stalled = torch.zeros(self.B, dtype=torch.int32, device=dev)
        self.iteration = 0
        self._traces, self._counts = [], []
        self._ws, self._caps = None, None

    # ------------------------------------------------------------------ what every call shares
    def _layout(self):
        return (L.ptr(self.dataset.images), L.ptr(self.dataset.depths), int(self.dataset.depths.dtype == torch.float16), L.ptr(self.dataset.semantics),
                int(self.dataset.semantics.dtype == torch.uint8), int(self.dataset.images.shape[0]), L.ptr(self.image_ids), L.ptr(self.c2w0),
                float(self.dataset._focal), self.W, self.H)

    def _workspace(self, handle):
        caps = RD._train_state(self.field).caps(self.B * self.n)
        lib = L.load_library()
        nbytes = int(lib.mnf_pose_refine_workspace_bytes(handle, self.B, self.n, *caps))
        if nbytes <= 0:
            raise L.MnfError("PoseRefiner: bad sizes for the workspace")
        if self._ws is None or self._caps != caps or self._ws.numel() < nbytes:
            self._ws, self._caps = torch.empty(nbytes, dtype=torch.uint8, device=self.xi.device), caps
        return self._ws, nbytes, caps

    @torch.no_grad()
    def step(self, n_iters=1):
        """Enqueue `n_iters` iterations on torch's current stream.  Returns nothing and does not wait for the GPU."""
        n_iters = int(n_iters)
        if n_iters <= 0:
            return
        lib, dev = L.load_library(), self.xi.device
        handle, grid = self.field._ensure_handle(), RD._grid_args(self.estimator)
        opts, _, bk_dev = RD._train_opts(self.field, grid, dev, seed=0, loss_scale=float(self.field.loss_scale), render_bkgd=self.render_bkgd, stratified=False,
                                         **self.render_kw)
        ws, nbytes, caps = self._workspace(handle)
        trace = torch.empty(n_iters, self.B, dtype=torch.float64, device=dev)
        counts = torch.empty(n_iters, 4, dtype=torch.int64, device=dev)
        L.launch(lib.mnf_pose_refine, handle, L.ptr(grid.binaries), L.ptr(grid.bits), L.ptr(grid.occs), *grid.res, grid.aabb, *self._layout(), L.ptr(self.pix_idx),
                 self.B, self.n, L.ptr(self.xi), L.ptr(self.adam_m), L.ptr(self.adam_v), self.iteration, n_iters, ctypes.byref(opts), ctypes.byref(self.pose),
                 L.ptr(trace), L.ptr(self.stalled), L.ptr(counts), *caps, L.ptr(ws), nbytes)
        self._keep = (grid, bk_dev)
        self.iteration += n_iters
        self._traces.append(trace)
        self._counts.append(counts)

    @torch.no_grad()
    def formed(self, iteration=None):
        """What `mnf_pose_rays` forms for `iteration` (default: the next one) at the current `xi`: dict(origins, viewdirs [B,n,3], pix [B,n], R [B,3,3],
        rgb [B,n,3], dep [B,n], sem [B,n]) as device tensors — the rays and targets an iteration of `step` starts from."""
        dev, B, n = self.xi.device, self.B, self.n
        it = self.iteration if iteration is None else int(iteration)
        o, d = torch.empty(B, n, 3, device=dev), torch.empty(B, n, 3, device=dev)
        pix, rot = torch.empty(B, n, dtype=torch.int64, device=dev), torch.empty(B, 3, 3, device=dev)
        rgb, dep, sem = torch.empty(B, n, 3, device=dev), torch.empty(B, n, device=dev), torch.empty(B, n, dtype=torch.int64, device=dev)
        L.launch(L.load_library().mnf_pose_rays, *self._layout(), L.ptr(self.pix_idx), L.ptr(self.xi), B, n, it, int(self.pose.seed), L.ptr(o), L.ptr(d), L.ptr(pix),
                 L.ptr(rot), L.ptr(rgb), L.ptr(dep), L.ptr(sem))
        return dict(origins=o, viewdirs=d, pix=pix, R=rot, rgb=rgb, dep=dep, sem=sem)

    def last_iteration(self, what):
        """A view of what the latest enqueued iteration left in the workspace (`WS_*`): rays, pixel ids, rendered planes, ray gradients, the 6-vector
        gradients, R.  For tests and tools; valid until the next `step`."""
        B, n, C = self.B, self.n, int(self.field.num_semantic_classes)
        if self._ws is None:
            raise L.MnfError("PoseRefiner.last_iteration: no iteration has been enqueued")
        off = int(L.load_library().mnf_pose_refine_workspace_offset(self.field._ensure_handle(), B, n, *self._caps, int(what)))
        shape, dtype = {WS_RAYS_O: ((B, n, 3), torch.float32), WS_RAYS_D: ((B, n, 3), torch.float32), WS_PIX: ((B, n), torch.int64),
                        WS_RGB: ((B, n, 3), torch.float32), WS_ACC: ((B, n), torch.float32), WS_DEPTH: ((B, n), torch.float32),
                        WS_SEM: ((B, n, C), torch.float32), WS_G_RAYS_O: ((B, n, 3), torch.float32), WS_G_RAYS_D: ((B, n, 3), torch.float32),
                        WS_GRAD: ((B, 6), torch.float64), WS_ROT: ((B, 3, 3), torch.float32), WS_KEPT: ((B, n), torch.int64)}[int(what)]
        count = int(np.prod(shape))
        return self._ws[off:off + count * torch.empty((), dtype=dtype).element_size()].view(dtype).view(shape)

    @torch.no_grad()
    def result(self):
        """One host copy -> dict(c2w [B,4,4] float64: the refined poses [R R0 | c + trans], xi [B,6], loss_trace [iterations,B], stalled [B] (iterations
        that left the view alone), status (the OR of every iteration's status bits: mnf_train_step's, 8 = a label outside the classes), counts
        [iterations,4])."""
        B, iters = self.B, self.iteration
        parts = [self.xi.reshape(-1), self.c2w0.to(torch.float64).reshape(-1), self.stalled.to(torch.float64)]
        parts += [t.reshape(-1) for t in self._traces] + [c.to(torch.float64).reshape(-1) for c in self._counts]
        host = torch.cat(parts).cpu().numpy()
        xi, c2w0, stalled = host[:6 * B].reshape(B, 6), host[6 * B:18 * B].reshape(B, 3, 4), host[18 * B:19 * B].astype(np.int64)
        trace = host[19 * B:19 * B + iters * B].reshape(iters, B)
        counts = host[19 * B + iters * B:].reshape(iters, 4).astype(np.int64)
        if len(self._traces) > 1:      # (kept as one block each: the next result() concatenates two tensors, not every step's)
            self._traces, self._counts = [torch.cat(self._traces)], [torch.cat(self._counts)]
        status = int(np.bitwise_or.reduce(counts[:, 3])) if iters else 0
        return dict(c2w=compose_c2w(c2w0, xi), xi=xi.copy(), loss_trace=trace.copy(), stalled=stalled, status=status, counts=counts)


def refine_poses(radiance_field, estimator, dataset, image_ids, c2w0=None, n_iters=50, **kw):
    """The one-call form: `PoseRefiner(...)`, `step(n_iters)`, `result()`."""
    ref = PoseRefiner(radiance_field, estimator, dataset, image_ids, c2w0, **kw)
    ref.step(n_iters)
    return ref.result()
