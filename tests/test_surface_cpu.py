"""The numpy restatement of the surface mesh, tests/surface_ref.py, held to the definition of include/mi355nerf.h ("surface mesh"): known
counts, areas and volumes, closed and consistently oriented meshes, the Euler characteristic of a ball, the edge cases of the inside test,
the open boundary, and the PLY writer of apnrf_amd.surface byte for byte.  No GPU: tests/test_gpu_surface.py holds the device to the
restatement."""
import math

import numpy as np
import pytest

import surface_ref as SR

ORIGIN0, STEP1 = (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)


@pytest.fixture(scope="module")
def meshes():
    """Each mesh is extracted once; the arrays are read-only."""
    cache = {}

    def get(name):
        if name not in cache:
            values = {"point": SR.single_point, "ball17": lambda: SR.ball((17, 17, 17), 5.3), "ball33": lambda: SR.ball((33, 33, 33), 11.7),
                      "ball_odd": lambda: SR.ball((17, 13, 11), 3.9), "torus_odd": lambda: SR.torus((17, 13, 11), 3.2, 1.4)}[name]()
            m = SR.extract(values, 0.5 if name == "point" else 0.0, ORIGIN0, STEP1)
            for k in ("positions", "normals", "triangles"):
                m[k].setflags(write=False)
            cache[name] = m
        return cache[name]
    return get


def test_workspace_byte_functions():
    """The two workspace layouts of the device unit (csrc/surface.hip), byte for byte; the functions need no GPU."""
    import __graft_entry__ as G
    import apnrf_amd
    G.build()
    lib = apnrf_amd.load_library()
    # a single cell, word counts that need padding to 8 bytes, a realistic lattice, the cap
    extract = {(1, 1, 1): 96, (2, 2, 2): 176, (16, 12, 10): 10080, (6, 4, 10): 1640, (196, 34, 196): 5603104, (1024, 1024, 1024): 4442190328}
    for cells, want in extract.items():
        assert lib.mnf_surface_extract_workspace_bytes(*cells) == want, cells
    points = {(1, 1, 1, 1): 48, (4, 3, 5, 2): 136, (3, 3, 3, 1): 72, (7, 5, 9, 4): 1768, (128, 128, 128, 1): 2231384, (196, 34, 196, 2): 1972392}
    for args, want in points.items():
        assert lib.mnf_surface_lattice_points_workspace_bytes(*args) == want, args
    assert lib.mnf_surface_extract_workspace_bytes(0, 1, 1) == 0 and lib.mnf_surface_lattice_points_workspace_bytes(4, 3, 5, 3) == 0


def _closed(m):
    return len(SR.boundary_edges(m["triangles"])) == 0


def test_one_inside_point(meshes):
    """A Kuhn lattice point has 14 neighbours and sits in 24 tetrahedra."""
    m = meshes("point")
    assert m["positions"].shape == (14, 3) and m["triangles"].shape == (24, 3)
    area, volume = SR.measure(m["positions"], m["triangles"])
    assert abs(area - 3.621320343559643) < 1e-12 and abs(volume - 0.5) < 1e-12       # midpoints: every coordinate is a multiple of 0.5
    assert _closed(m) and SR.euler_characteristic(14, m["triangles"]) == 2
    # the lattice differences of a single point vanish at its diagonal neighbours: those 8 normals are (0,0,0), the 6 on the axes point outwards
    out = m["positions"] - np.array([2.0, 2.0, 2.0])
    length = np.linalg.norm(m["normals"].astype(np.float64), axis=1)
    assert sorted(length.tolist()) == [0.0] * 8 + [1.0] * 6
    assert np.array_equal(m["normals"][length > 0], 2 * out[length > 0])


@pytest.mark.parametrize("name,radius,nv,nt,area_ratio,volume_ratio", [("ball17", 5.3, 1598, 3192, 0.990782, 0.982136), ("ball33", 11.7, 7730, 15456, 0.998119, 0.996349)])
def test_ball(meshes, name, radius, nv, nt, area_ratio, volume_ratio):
    """Counts exactly.  The ratios to the exact sphere are what this restatement was measured to give, to six decimals (they round to the
    four decimals 0.9908 / 0.9821 and 0.9981 / 0.9963 recorded before it existed), within 1e-6: half a unit of the last recorded decimal,
    far above the 1e-12 that float64 sums of a few thousand terms of this size can differ by."""
    m = meshes(name)
    assert (len(m["positions"]), len(m["triangles"])) == (nv, nt)
    area, volume = SR.measure(m["positions"], m["triangles"])
    ra, rv = area / (4.0 * math.pi * radius ** 2), volume / (4.0 / 3.0 * math.pi * radius ** 3)
    print(f"{name}: area ratio {ra:.6f}, volume ratio {rv:.6f}")
    assert abs(ra - area_ratio) <= 1e-6 and abs(rv - volume_ratio) <= 1e-6
    assert _closed(m) and SR.euler_characteristic(nv, m["triangles"]) == 2
    e = SR.directed_edges(m["triangles"])
    assert len(np.unique(e, axis=0)) == len(e)                                       # each directed edge once (and, closed, its reverse once)
    centre = (np.array([17 if name == "ball17" else 33] * 3) - 1.0) / 2.0 + 0.13
    radial = m["positions"] - centre
    radial /= np.linalg.norm(radial, axis=1, keepdims=True)
    assert (np.einsum("ij,ij->i", radial, m["normals"].astype(np.float64)) > 0.99).all()   # the normals point out of the matter


def test_shapes_inside_their_lattice_are_closed_and_every_case_occurs(meshes):
    ball, torus = meshes("ball_odd"), meshes("torus_odd")
    assert _closed(ball) and _closed(torus)
    assert SR.euler_characteristic(len(ball["positions"]), ball["triangles"]) == 2
    assert SR.euler_characteristic(len(torus["positions"]), torus["triangles"]) == 0
    assert ball["cases"] | torus["cases"] == {(k, s) for k in range(6) for s in range(1, 15)}   # the 14 sign cases of each tetrahedron
    area, volume = SR.measure(torus["positions"], torus["triangles"])
    assert volume > 0 and abs(volume / (2 * math.pi ** 2 * 3.2 * 1.4 ** 2) - 1) < 0.1  # outward orientation: the volume is positive


def test_orientation_table_is_outward():
    """Each case of each tetrahedron: triangle normals (crossings at edge midpoints) point from the inside to the outside mean."""
    for k in range(6):
        V = SR.tet_vertices(k).astype(np.float64)
        for s in range(1, 15):
            ins = [i for i in range(4) if (s >> i) & 1]
            outs = [i for i in range(4) if not (s >> i) & 1]
            w = V[outs].mean(axis=0) - V[ins].mean(axis=0)
            tris = SR.CASES[k][s]
            assert len(tris) == (2 if len(ins) == 2 else 1)
            for tri in tris:
                assert all((i in ins) != (j in ins) for i, j in tri)
                q = [0.5 * (V[i] + V[j]) for i, j in tri]
                assert np.dot(np.cross(q[1] - q[0], q[2] - q[0]), w) > 0
    assert SR.CASES[0][1] == [[(0, 1), (0, 2), (0, 3)]] or SR.CASES[0][1] == [[(0, 1), (0, 3), (0, 2)]]


def test_iso_equal_to_a_value_nan_and_inf():
    v = SR.single_point()
    on = SR.extract(v, 1.0, ORIGIN0, STEP1)                                            # a value equal to iso is outside
    assert len(on["positions"]) == 0 and len(on["triangles"]) == 0
    v2 = SR.ball((9, 9, 9), 2.6)
    v2[4, 4, 4] = np.float32(0.25)
    m = SR.extract(v2, 0.25, ORIGIN0, STEP1)                                           # the centre counts as outside: a cavity
    plain = SR.extract(SR.ball((9, 9, 9), 2.6), 0.25, ORIGIN0, STEP1)
    assert len(m["positions"]) == len(plain["positions"]) + 14 and len(m["triangles"]) == len(plain["triangles"]) + 24 and _closed(m)
    # t runs from the owner: 0 / (b - a) = 0 on the 7 edges the on-iso point owns, (iso - a) / (iso - a) = 1 on the 7 it ends: all 14 sit on it
    own = np.all(m["positions"] == np.array([4, 4, 4], np.float32), axis=1)
    assert own.sum() == 14
    for bad in (np.nan, np.inf, -np.inf):
        v3 = SR.ball((9, 9, 9), 2.6)
        v3[4, 4, 4] = bad
        v3[1, 1, 1] = bad
        m3 = SR.extract(v3, 0.25, ORIGIN0, STEP1)
        assert np.isfinite(m3["positions"]).all() and np.isfinite(m3["normals"]).all() and _closed(m3)
        inside = bad == np.inf
        # +inf is inside (the ball stays whole, an island appears at (1,1,1)); NaN and -inf are outside (a cavity, nothing at (1,1,1))
        assert len(m3["triangles"]) == len(plain["triangles"]) + 24
        frac = m3["positions"] - np.floor(m3["positions"])
        near = np.abs(m3["positions"] - np.array([1, 1, 1] if inside else [4, 4, 4], np.float32)).max(axis=1) <= 1
        assert near.sum() == 14 and np.isin(frac[near], (0.0, 0.5)).all()              # t = 0.5f on every edge with a non-finite end


def test_slab_is_open_at_the_boundary_only():
    v = np.full((7, 6, 9), -1.0, np.float32)
    v[2:4] = 1.0                                                                       # a slab across y and z, two points thick in x
    m = SR.extract(v, 0.0, (1.0, -2.0, 0.5), (0.5, 0.25, 2.0))
    b = SR.boundary_edges(m["triangles"])
    assert len(b) > 0
    p = m["positions"][b.reshape(-1)]
    lo, hi = np.array([1.0, -2.0, 0.5]), np.array([1.0 + 6 * 0.5, -2.0 + 5 * 0.25, 0.5 + 8 * 2.0])
    on_side = (p[:, 1] == lo[1]) | (p[:, 1] == hi[1]) | (p[:, 2] == lo[2]) | (p[:, 2] == hi[2])
    assert on_side.all()                                                               # every open edge lies on the lattice boundary
    assert set(np.unique(m["positions"][:, 0]).tolist()) == {1.0 + 1.5 * 0.5, 1.0 + 3.5 * 0.5}
    assert np.array_equal(np.abs(m["normals"]), np.tile(np.array([1, 0, 0], np.float32), (len(m["normals"]), 1)))
    inner = SR.extract(np.pad(v, 1, constant_values=-1.0), 0.0, ORIGIN0, STEP1)         # the same slab strictly inside: closed
    assert _closed(inner)


def test_sliver_and_anisotropic_step():
    v = np.array([[[1.0, -1.0], [-3.0, -1.0]], [[-1.0, -2.0], [-1.0, -1.0]], [[-1.0, -1.0], [-1.0, 5.0]]], np.float32)   # 2 x 1 x 1 cells
    m = SR.extract(v, 0.0, (0.0, 0.0, 0.0), (1.0, 2.0, 4.0))
    assert len(m["positions"]) == 7 + 7 and len(m["triangles"]) == 6 + 6               # a corner of one cell cut off by each of its tetrahedra, twice
    assert m["positions"][0].tolist() == [0.5, 0.0, 0.0]                               # (p, type 0): t = 0.5
    assert m["positions"][1].tolist() == [0.0, 0.5, 0.0]                               # (p, type 1): t = 1 / 4, y = 0.25 * 2
    assert m["positions"][2].tolist() == [0.0, 0.0, 2.0]                               # (p, type 2): t = 0.5, z = 0.5 * 4


def test_lattice_points_and_attrs_restatement():
    b = np.zeros((4, 3, 5), bool)
    b[0, 0, 0] = True
    lin, pos, origin, step, shape = SR.lattice_points(b, 2, (0.0, 0.0, 0.0, 4.0, 3.0, 5.0))
    assert shape == (9, 7, 11) and len(lin) == 5 * 5 * 5 and (np.diff(lin) > 0).all()   # cells 0..1 per axis: points 0..4
    assert step.tolist() == [0.5, 0.5, 0.5] and pos.max() == 2.0
    assert len(SR.lattice_points(np.zeros((4, 3, 5), bool), 1, (0, 0, 0, 1, 1, 1))[0]) == 0
    a = SR.vertex_attrs(np.array([[0.5, -1.0, 2.0], [np.nan, 1.0, 0.0]], np.float32), np.array([[1.0, 3.0, 3.0], [0.0, np.nan, 1.0]], np.float32),
                        np.array([[1, 2, 3], [4, 5, 6], [7, 8, 9]], np.uint8))
    assert a["colour"].tolist() == [[128, 0, 255], [0, 255, 0]] and a["label"].tolist() == [1, -1]
    assert a["sem_colour"].tolist() == [[4, 5, 6], [0, 0, 0]]


def test_ply_round_trip_byte_for_byte(tmp_path, meshes):
    import torch
    from apnrf_amd.surface import SurfaceMesh, load_ply
    m = meshes("ball17")
    nv = len(m["positions"])
    rng = np.random.default_rng(3)
    colour = rng.integers(0, 256, (nv, 3)).astype(np.uint8)
    label = rng.integers(-1, 29, nv).astype(np.int32)
    mesh = SurfaceMesh(torch.from_numpy(m["positions"].copy()), torch.from_numpy(m["normals"].copy()), torch.from_numpy(m["triangles"].copy()),
                       torch.tensor([nv, len(m["triangles"]), 0, 0]), colour=torch.from_numpy(colour), label=torch.from_numpy(label))
    path = str(tmp_path / "ball.ply")
    mesh.save_ply(path)
    got = load_ply(path)
    for k, want in (("positions", m["positions"]), ("normals", m["normals"]), ("triangles", m["triangles"]), ("colour", colour), ("label", label)):
        assert got[k].dtype == want.dtype and got[k].tobytes() == want.tobytes(), k
    data = open(path, "rb").read()
    head = data[:data.index(b"end_header\n") + 11]
    assert head.startswith(b"ply\nformat binary_little_endian 1.0\n") and f"element vertex {nv}\n".encode() in head
    assert len(data) == len(head) + nv * 31 + len(m["triangles"]) * 13                 # 6 floats + 3 bytes + int32; uchar + 3 int32
    body = data[len(head):]
    assert body[:12] == m["positions"][0].tobytes() and body[24:27] == colour[0].tobytes() and body[27:31] == label[0].tobytes()
    assert body[nv * 31:nv * 31 + 13] == b"\x03" + m["triangles"][0].astype("<i4").tobytes()
    again = str(tmp_path / "again.ply")
    SurfaceMesh(*[torch.from_numpy(got[k]) for k in ("positions", "normals", "triangles")], mesh.info, colour=torch.from_numpy(got["colour"]),
                label=torch.from_numpy(got["label"])).save_ply(again)
    assert open(again, "rb").read() == data
    bare = str(tmp_path / "bare.ply")                                                  # no attributes: black, label -1
    SurfaceMesh(mesh.positions, mesh.normals, mesh.triangles, mesh.info).save_ply(bare)
    g = load_ply(bare)
    assert (g["label"] == -1).all() and (g["colour"] == 0).all() and g["triangles"].tobytes() == m["triangles"].tobytes()


def test_ply_of_an_empty_mesh(tmp_path):
    import torch
    from apnrf_amd.surface import SurfaceMesh, load_ply
    mesh = SurfaceMesh(torch.empty(0, 3), torch.empty(0, 3), torch.empty(0, 3, dtype=torch.int32), torch.zeros(4, dtype=torch.int64),
                       colour=torch.empty(0, 3, dtype=torch.uint8), label=torch.empty(0, dtype=torch.int32))
    path = str(tmp_path / "empty.ply")
    mesh.save_ply(path)
    data = open(path, "rb").read()
    assert data.endswith(b"end_header\n") and b"element vertex 0\n" in data and b"element face 0\n" in data
    got = load_ply(path)
    assert got["positions"].shape == (0, 3) and got["normals"].shape == (0, 3) and got["colour"].shape == (0, 3)
    assert got["label"].shape == (0,) and got["triangles"].shape == (0, 3)
