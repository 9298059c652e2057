"""The semantic surface mesh of a trained field, extracted on the device (csrc/surface.hip): the iso-surface of the field's density over a
lattice refined from the estimator's occupancy grid, by marching tetrahedra, with a colour, a normal and a semantic class per vertex.
What the `extract_mesh` of the reference's nerfacc benchmarks does with a host package, and what the semantic ground-truth cloud of
simulator/build_point_cloud_from_mesh.py is compared with.  Only the finished mesh visits the host (`SurfaceMesh.cpu`, `save_ply`).
The definition is in include/mi355nerf.h ("surface mesh") and DESIGN.md."""
import ctypes

import numpy as np
import torch

from . import _lib as L

_PLY_VERTEX = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4"), ("red", "u1"), ("green", "u1"),
                        ("blue", "u1"), ("label", "<i4")])
_PLY_FACE = np.dtype([("n", "u1"), ("v", "<i4", (3,))])


def _f3(v):
    a = np.asarray(v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v, np.float32).reshape(3)
    return (ctypes.c_float * 3)(*[float(x) for x in a]), a


class SurfaceMesh:
    """positions, normals [V,3] float32, triangles [T,3] int32 (vertex indices, outward orientation), and where the field was asked:
    colour [V,3] uint8, label [V] int32 (-1: a NaN logit), sem_colour [V,3] uint8.  `info` is the int64 [4] of mnf_surface_extract."""

    def __init__(self, positions, normals, triangles, info, colour=None, label=None, sem_colour=None):
        self.positions, self.normals, self.triangles, self.info = positions, normals, triangles, info
        self.colour, self.label, self.sem_colour = colour, label, sem_colour

    @property
    def n_vertices(self):
        return int(self.positions.shape[0])

    @property
    def n_triangles(self):
        return int(self.triangles.shape[0])

    def measure_device(self):
        """float64 device tensor [2] = {area, enclosed volume}; does not synchronise."""
        L.require_gpu(self.positions, self.triangles)
        dev = self.positions.device
        nv, nt = self.n_vertices, self.n_triangles
        counts = self.info if self.info is not None and self.info.is_cuda else torch.tensor([nv, nt, 0, 0], dtype=torch.int64, device=dev)
        out = torch.empty(2, dtype=torch.float64, device=dev)
        L.launch(L.load_library().mnf_surface_measure, L.ptr(self.positions) if nv else None, L.ptr(self.triangles) if nt else None, L.ptr(counts), nv, nt,
                 L.ptr(out))
        return out

    def measure(self):
        """dict(area, volume) in float64: each triangle adds |(b - a) x (c - a)| / 2 and a . (b x c) / 6.  The volume means something
        for a closed mesh only."""
        area, volume = (float(v) for v in self.measure_device().cpu().numpy())
        return {"area": area, "volume": volume}

    def quality(self, gt_points, **kw):
        """`cloud.mesh_quality(self, gt_points, ...)`: accuracy, completion, F-score and class confusion against a ground-truth cloud."""
        from . import cloud
        return cloud.mesh_quality(self, gt_points, **kw)

    def cpu(self):
        """The same mesh on the host."""
        return SurfaceMesh(*[None if t is None else t.cpu() for t in (self.positions, self.normals, self.triangles, self.info, self.colour, self.label,
                                                                      self.sem_colour)])

    def save_ply(self, path):
        """Binary little-endian PLY: vertices x y z nx ny nz red green blue label (float32 x 6, uchar x 3, int32), faces uchar 3 + int32 x 3.
        Without attributes the colour is (0,0,0) and the label -1."""
        m = self.cpu()
        nv, nt = m.n_vertices, m.n_triangles
        v = np.zeros(nv, _PLY_VERTEX)
        pos, nrm = m.positions.numpy(), m.normals.numpy()
        for k, (a, b) in enumerate((("x", "nx"), ("y", "ny"), ("z", "nz"))):
            v[a], v[b] = pos[:, k], nrm[:, k]
        if m.colour is not None:
            c = m.colour.numpy()
            v["red"], v["green"], v["blue"] = c[:, 0], c[:, 1], c[:, 2]
        v["label"] = m.label.numpy() if m.label is not None else -1
        f = np.zeros(nt, _PLY_FACE)
        f["n"] = 3
        f["v"] = m.triangles.numpy()
        header = ("ply\nformat binary_little_endian 1.0\ncomment apnrf_amd surface mesh\n"
                  f"element vertex {nv}\nproperty float x\nproperty float y\nproperty float z\nproperty float nx\nproperty float ny\nproperty float nz\n"
                  "property uchar red\nproperty uchar green\nproperty uchar blue\nproperty int label\n"
                  f"element face {nt}\nproperty list uchar int vertex_indices\nend_header\n")
        with open(path, "wb") as fh:
            fh.write(header.encode("ascii"))
            fh.write(v.tobytes())
            fh.write(f.tobytes())


def load_ply(path):
    """The numpy reader of `save_ply`'s files -> dict(positions, normals f32 [V,3], colour u8 [V,3], label i32 [V], triangles i32 [T,3])."""
    with open(path, "rb") as fh:
        data = fh.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    lines = data[:end].decode("ascii").split("\n")
    if lines[0] != "ply" or lines[1] != "format binary_little_endian 1.0":
        raise ValueError(f"{path} is not a binary little-endian PLY")
    counts = {ln.split()[1]: int(ln.split()[2]) for ln in lines if ln.startswith("element ")}
    props = [ln for ln in lines if ln.startswith("property ")]
    want = ["property float " + n for n in ("x", "y", "z", "nx", "ny", "nz")] + ["property uchar " + n for n in ("red", "green", "blue")] + \
           ["property int label", "property list uchar int vertex_indices"]
    if props != want:
        raise ValueError(f"{path} does not have the layout save_ply writes")
    nv, nt = counts["vertex"], counts["face"]
    if len(data) != end + nv * _PLY_VERTEX.itemsize + nt * _PLY_FACE.itemsize:
        raise ValueError(f"{path}: {len(data)} bytes for {nv} vertices and {nt} faces")
    v = np.frombuffer(data, _PLY_VERTEX, nv, end)
    f = np.frombuffer(data, _PLY_FACE, nt, end + nv * _PLY_VERTEX.itemsize)
    if nt and not (f["n"] == 3).all():
        raise ValueError(f"{path}: a face that is not a triangle")
    return {"positions": np.stack([v["x"], v["y"], v["z"]], axis=1), "normals": np.stack([v["nx"], v["ny"], v["nz"]], axis=1),
            "colour": np.stack([v["red"], v["green"], v["blue"]], axis=1), "label": v["label"].copy(), "triangles": f["v"].copy()}


def _extract_call(values, cells, iso, origin, step, max_v, max_t, observed=False):
    lib = L.load_library()
    dev = values.device
    nbytes = int(lib.mnf_surface_extract_workspace_bytes(*cells))
    if nbytes <= 0:
        raise L.MnfError(f"a lattice of {cells[0]} x {cells[1]} x {cells[2]} cells is outside 1 .. 1024 per axis")
    pos = torch.empty(max_v, 3, dtype=torch.float32, device=dev)
    nrm = torch.empty(max_v, 3, dtype=torch.float32, device=dev)
    tri = torch.empty(max_t, 3, dtype=torch.int32, device=dev)
    info = torch.empty(4, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        # a plain temporary, not the per-stream workspace cache: it is lattice-sized (4.1 B per point: 557 MB for 513^3) and a one-off mesh
        # export must not pin that through later training or rendering; torch's allocator takes it back when the call's tensors go
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        L.launch(lib.mnf_surface_extract_observed if observed else lib.mnf_surface_extract, L.ptr(values), *cells, float(iso), origin, step, max_v, max_t, L.ptr(pos) if max_v else None,
                 L.ptr(nrm) if max_v else None, L.ptr(tri) if max_t else None, L.ptr(info), L.ptr(ws), nbytes)
    return pos, nrm, tri, info


@torch.no_grad()
def extract_lattice_surface(values, iso, origin, step, max_vertices=None, max_triangles=None, observed=False):
    """The iso-surface of a float32 device lattice `values` [X+1, Y+1, Z+1] (x slowest) by marching tetrahedra: a point is inside where
    value > iso; vertex positions are (index + t) * step + origin.  -> SurfaceMesh of device tensors cut to the counts.  With no
    capacity given, a counting pass sizes the outputs (one small host copy); a given capacity that overflows raises an MnfError that
    names the count and the capacity.  The mesh is open where matter touches the lattice boundary.  `observed=True` takes a NaN point as
    UNOBSERVED instead of outside (`mnf_surface_extract_observed`, what a TSDF lattice needs): no edge with a NaN end carries a vertex and
    no tetrahedron with a NaN corner a triangle, so the mesh is open where nothing was observed; a vertex no triangle uses may remain."""
    L.require_gpu(values)
    if values.dim() != 3:
        raise ValueError(f"values is [X+1, Y+1, Z+1] (got {tuple(values.shape)})")
    v = L.contig(values, torch.float32)
    cells = tuple(int(n) - 1 for n in v.shape)
    o, _ = _f3(origin)
    s, _ = _f3(step)
    if max_vertices is None or max_triangles is None:
        counts = _extract_call(v, cells, iso, o, s, 0, 0, observed)[3].cpu().numpy()
        max_vertices = int(counts[0]) if max_vertices is None else int(max_vertices)
        max_triangles = int(counts[1]) if max_triangles is None else int(max_triangles)
    max_vertices, max_triangles = int(max_vertices), int(max_triangles)
    pos, nrm, tri, info = _extract_call(v, cells, iso, o, s, max_vertices, max_triangles, observed)
    host = info.cpu().numpy()
    if host[2] or host[3]:
        raise L.MnfError(f"the surface has {int(host[0])} vertices and {int(host[1])} triangles: more than max_vertices = {max_vertices} / "
                         f"max_triangles = {max_triangles}")
    return SurfaceMesh(pos[:int(host[0])], nrm[:int(host[0])], tri[:int(host[1])], info)


def _lattice_points(binaries, refine, aabb6, max_points):
    lib = L.load_library()
    dev = binaries.device
    R = tuple(int(n) for n in binaries.shape)
    nbytes = int(lib.mnf_surface_lattice_points_workspace_bytes(*R, int(refine)))
    if nbytes <= 0:
        raise L.MnfError(f"refine = {refine} of a {R[0]} x {R[1]} x {R[2]} grid: refine is 1, 2, 4 or 8 and resolution x refine at most 1024 per axis")
    lin = torch.empty(max_points, dtype=torch.int32, device=dev)
    pos = torch.empty(max_points, 3, dtype=torch.float32, device=dev)
    info = torch.empty(2, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)        # a temporary, as in _extract_call
        L.launch(lib.mnf_surface_lattice_points, L.ptr(binaries), *R, int(refine), aabb6, max_points, L.ptr(lin) if max_points else None,
                 L.ptr(pos) if max_points else None, L.ptr(info), L.ptr(ws), nbytes)
    return lin, pos, info


@torch.no_grad()
def lattice_points(binaries, refine, aabb, max_points=None):
    """The points of the (R * refine + 1)^3 lattice over `aabb` that touch an occupied cell of `binaries` [RX, RY, RZ] or a cell next to
    one (3 x 3 x 3) -> dict(lin int32 [n] ascending, positions float32 [n,3], info int64 [2]) on the device.  With no capacity given a
    counting pass sizes the list (one small host copy)."""
    L.require_gpu(binaries)
    b = binaries.contiguous()
    b = b.view(torch.uint8) if b.dtype == torch.bool else b.to(torch.uint8)
    a = np.asarray(aabb.detach().cpu().numpy() if isinstance(aabb, torch.Tensor) else aabb, np.float32).reshape(6)
    aabb6 = (ctypes.c_float * 6)(*[float(x) for x in a])
    if max_points is None:
        max_points = int(_lattice_points(b, refine, aabb6, 0)[2].cpu().numpy()[0])
    lin, pos, info = _lattice_points(b, refine, aabb6, int(max_points))
    host = info.cpu().numpy()
    if host[1]:
        raise L.MnfError(f"{int(host[0])} lattice points exceed max_points = {int(max_points)}")
    n = int(host[0])
    return {"lin": lin[:n], "positions": pos[:n], "info": info}


def lattice_frame(aabb, resolution, refine):
    """(origin, step) float32 [3] of the refined lattice: origin = aabb_min, step = (aabb_max - aabb_min) / (float)(R * refine)."""
    a = np.asarray(aabb.detach().cpu().numpy() if isinstance(aabb, torch.Tensor) else aabb, np.float32).reshape(6)
    cells = np.array([int(r) * int(refine) for r in resolution]).astype(np.float32)
    return a[:3].copy(), ((a[3:] - a[:3]) / cells).astype(np.float32)


@torch.no_grad()
def lattice_from_field(radiance_field, estimator, refine=1):
    """The density lattice of a trained field: (values float32 [RX * refine + 1, ...] on the device, origin, step).  The field is asked
    (`query_density`, the field's own kernel) only at the lattice points that touch a cell the estimator holds occupied at level 0, or
    a cell next to one; every other point is 0, below any iso > 0."""
    b = estimator.binaries[0]
    L.require_gpu(b)
    aabb = estimator.aabbs[0]
    pts = lattice_points(b, refine, aabb)
    shape = tuple(int(n) * int(refine) + 1 for n in b.shape)
    n = int(pts["lin"].shape[0])
    values = torch.empty(shape, dtype=torch.float32, device=b.device)
    density = radiance_field.query_density(pts["positions"]).reshape(-1).contiguous() if n else None
    L.launch(L.load_library().mnf_surface_lattice_scatter, L.ptr(density), L.ptr(pts["lin"]) if n else None, L.ptr(pts["info"]), n, L.ptr(values),
             values.numel())
    origin, step = lattice_frame(aabb, b.shape, refine)
    return values, origin, step


@torch.no_grad()
def vertex_attrs(rgb, sem, palette=None):
    """rgb [n,3], sem [n,C] float32 device tensors (the field's outputs) -> dict(colour uint8 [n,3], label int32 [n], and with a
    `palette` [K,3] uint8, K >= C: sem_colour uint8 [n,3]).  One launch, no host copy."""
    L.require_gpu(rgb, sem, palette)
    rgb = L.contig(rgb.reshape(-1, 3), torch.float32)
    n, C = int(rgb.shape[0]), int(sem.shape[-1])                     # C from sem's own last dimension: n may be 0
    sem = L.contig(sem.reshape(n, C), torch.float32)
    dev = rgb.device
    out = {"colour": torch.empty(n, 3, dtype=torch.uint8, device=dev), "label": torch.empty(n, dtype=torch.int32, device=dev)}
    pal = None
    if palette is not None:
        pal = L.contig(palette, torch.uint8)
        if pal.dim() != 2 or int(pal.shape[0]) < C or int(pal.shape[1]) != 3:
            raise ValueError(f"palette is [K, 3] with K >= {C} (got {tuple(pal.shape)})")
        out["sem_colour"] = torch.empty(n, 3, dtype=torch.uint8, device=dev)
    if n:
        L.launch(L.load_library().mnf_surface_vertex_attrs, L.ptr(rgb), L.ptr(sem), n, C, L.ptr(pal), L.ptr(out["colour"]), L.ptr(out["label"]),
                 L.ptr(out.get("sem_colour")))
    return out


@torch.no_grad()
def extract_surface(radiance_field, estimator, iso, refine=1, palette=None, max_vertices=None, max_triangles=None):
    """The whole route: the density lattice of the field (`lattice_from_field`), its iso-surface (`extract_lattice_surface`),
    `radiance_field.forward(positions, -normals)` at the vertices (the colour seen from outside, along the inward normal), and the
    attributes (`vertex_attrs`).  -> SurfaceMesh on the device.

    `iso` is a density.  The natural choice is the density at which the estimator calls a cell occupied, occ_thre / render_step_size
    (the estimator thresholds density * render_step_size at occ_thre); it must be > 0 for the unevaluated part of the lattice to stay
    outside."""
    values, origin, step = lattice_from_field(radiance_field, estimator, refine)
    mesh = extract_lattice_surface(values, iso, origin, step, max_vertices, max_triangles)
    if mesh.n_vertices:
        rgb, _, sem = radiance_field.forward(mesh.positions, -mesh.normals)
    else:
        rgb = torch.empty(0, 3, dtype=torch.float32, device=values.device)
        sem = torch.empty(0, int(radiance_field.num_semantic_classes), dtype=torch.float32, device=values.device)
    if palette is not None and not isinstance(palette, torch.Tensor):
        palette = torch.from_numpy(np.ascontiguousarray(palette, np.uint8))
    if palette is not None:
        palette = palette.to(values.device)
    a = vertex_attrs(rgb, sem, palette)
    mesh.colour, mesh.label, mesh.sem_colour = a["colour"], a["label"], a.get("sem_colour")
    return mesh
