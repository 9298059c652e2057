"""GPU tests of the scene sensor (csrc/sensor.hip, apnrf_amd/sensor.py) against the numpy restatement tests/sensor_ref.py, which
tests/test_sensor_cpu.py holds to brute force.  Every call goes through the C ABI with canaries on both sides of every output, twice, and the
two runs must give the same bytes.  hit, face, rgba, sem, planar depth and the float64 t_hit are `array_equal` to the restatement: both
sides round every float64 operation separately and in the same order.  Ray-mode depth is compared within one float32 ulp: the device's
square root is assumed correctly rounded, not bit-equal to numpy's."""
import ctypes

import numpy as np
import pytest
import torch

import sensor_ref as SR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CANARY = 64
MARKS = {torch.uint8: 0xA5, torch.int32: -0x5A5A5A5B, torch.int64: -0x5A5A5A5A5A5A5A5B, torch.float32: -12345.5, torch.float64: -12345.5}


def _dev(a):
    return torch.from_numpy(np.array(a, copy=True, order="C")).to(DEV)


def _guarded(n, dtype):
    whole = torch.full((n + 2 * CANARY,), MARKS[dtype], dtype=dtype, device=DEV)
    return whole, whole[CANARY:CANARY + n]


def _assert_guards(whole, n, what):
    host, mark = whole.cpu().numpy(), MARKS[whole.dtype]
    assert (host[:CANARY] == mark).all() and (host[CANARY + n:] == mark).all(), f"{what}: written outside its bounds"


def _lib():
    from apnrf_amd import _lib as L
    return L, L.load_library()


def _c3(v):
    return (ctypes.c_double * 3)(*[float(x) for x in v])


def _shade(v=SR.SHADE):
    return (ctypes.c_uint8 * 7)(*[int(x) for x in v])


class GpuScene:
    """A scene of the restatement on the device, its brick mask built through the C ABI (twice, guarded) and held to the restatement's."""

    def __init__(self, voxels, lo, s):
        L, lib = _lib()
        self.host, self.lo, self.s = voxels, np.asarray(lo, np.float64), float(s)
        self.shape = voxels.shape
        self.voxels = _dev(voxels.view(np.int32))
        words = int(lib.mnf_sensor_bricks_words(*self.shape))
        assert words == SR.bricks_words(self.shape)
        outs = []
        for _ in range(2):
            whole, bricks = _guarded(words, torch.int32)
            L.launch(lib.mnf_sensor_build_bricks, L.ptr(self.voxels), *self.shape, L.ptr(bricks), device=torch.device(DEV))
            torch.cuda.synchronize()
            _assert_guards(whole, words, "bricks")
            outs.append(bricks.cpu().numpy().view(np.uint32))
        assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], SR.build_bricks(voxels))
        self.bricks = bricks

    def args(self):
        L, _ = _lib()
        return (L.ptr(self.voxels), *self.shape, L.ptr(self.bricks), _c3(self.lo), self.s)


LO, S = np.array([-1.3, -0.2, 0.7]), 0.05
FREE = np.uint32(0xFF000000)
GRIDS = {
    "19x9x21": lambda: SR.clutter_grid((19, 9, 21), 0.03, 5),
    "8x8x8": lambda: SR.clutter_grid((8, 8, 8), 0.05, 6, floor=False),                 # one brick
    "70x9x40": lambda: SR.clutter_grid((70, 9, 40), 0.01, 7),                          # 9 x 2 x 5 bricks: more than one 32-bit word
    "all_free": lambda: np.full((11, 9, 10), FREE, np.uint32),
    "all_occupied": lambda: SR.pack(*np.random.default_rng(1).integers(0, 256, size=(3, 9, 5, 10)), np.random.default_rng(2).integers(0, 29, size=(9, 5, 10))),
}
_SCENES = {}


def gpu_scene(name):
    if name not in _SCENES:
        v = GRIDS[name]()
        v.setflags(write=False)
        _SCENES[name] = GpuScene(v, LO, S)
    return _SCENES[name]


def gpu_cast(sc, o, d, near, far):
    L, lib = _lib()
    n = o.shape[0]
    d_o, d_d = _dev(o), _dev(d)
    outs = []
    for _ in range(2):
        tw, t = _guarded(n, torch.float64)
        hw, h = _guarded(n, torch.int32)
        fw, f = _guarded(n, torch.uint8)
        iw, info = _guarded(2, torch.int64)
        info.zero_()
        L.launch(lib.mnf_sensor_cast_rays, *sc.args(), L.ptr(d_o), L.ptr(d_d), n, near, far, L.ptr(t), L.ptr(h), L.ptr(f), L.ptr(info), device=torch.device(DEV))
        torch.cuda.synchronize()
        for w, k, what in ((tw, n, "t_hit"), (hw, n, "hit"), (fw, n, "face"), (iw, 2, "info")):
            _assert_guards(w, k, what)
        outs.append([x.cpu().numpy() for x in (t, h, f, info)])
    assert all(a.tobytes() == b.tobytes() for a, b in zip(*outs))
    return outs[0]


def gpu_views(sc, c2w, W, H, focal, near, far, ray_depth=False, want_hit=True, shade=SR.SHADE, background=SR.BACKGROUND):
    L, lib = _lib()
    c2w = np.ascontiguousarray(np.asarray(c2w, np.float64).reshape(-1, 3, 4))
    V = c2w.shape[0]
    P = V * H * W
    d_m = _dev(c2w) if V else None
    outs = []
    for _ in range(2):
        rw, rgba = _guarded(4 * P, torch.uint8)
        dw, dep = _guarded(P, torch.float32)
        sw, sem = _guarded(P, torch.uint8)
        hw, hit = _guarded(P, torch.int32)
        iw, info = _guarded(2, torch.int64)
        info.zero_()
        L.launch(lib.mnf_sensor_views, *sc.args(), L.ptr(d_m), V, W, H, float(focal), near, far, int(ray_depth), _shade(shade), background, L.ptr(rgba), L.ptr(dep),
                 L.ptr(sem), L.ptr(hit) if want_hit else None, L.ptr(info), device=torch.device(DEV))
        torch.cuda.synchronize()
        for w, k, what in ((rw, 4 * P, "rgba"), (dw, P, "depth"), (sw, P, "sem"), (hw, P, "hit"), (iw, 2, "info")):
            _assert_guards(w, k, what)
        if not want_hit:
            assert (hit.cpu().numpy() == MARKS[torch.int32]).all()
        outs.append({"rgba": rgba.cpu().numpy().reshape(V, H, W, 4), "depth": dep.cpu().numpy().reshape(V, H, W), "sem": sem.cpu().numpy().reshape(V, H, W),
                     "hit": hit.cpu().numpy().reshape(V, H, W), "info": info.cpu().numpy()})
    assert all(outs[0][k].tobytes() == outs[1][k].tobytes() for k in outs[0])
    return outs[0]


# ------------------------------------------------------------------ the walk
@pytest.mark.parametrize("name", list(GRIDS))
def test_cast_rays_equal_the_restatement(name):
    sc = gpu_scene(name)
    o, d = SR.ray_mix(sc.shape, LO, S, n=700, seed=21)
    lo_l, lo_d = SR.lattice_rays(sc.shape, LO, S)
    o, d = np.concatenate([o, lo_l, [[np.nan, 0, 0], [0, 0, 1.0]]]), np.concatenate([d, lo_d, [[0, -1.0, 0], [np.inf, 0, 0]]])
    for near, far in ((0.0, 100.0), (0.3, 0.8)):
        t, hit, face, bad = SR.walk(sc.host, LO, S, o, d, near, far)
        gt, gh, gf, info = gpu_cast(sc, o, d, near, far)
        np.testing.assert_array_equal(gh, hit, err_msg=name)
        np.testing.assert_array_equal(gf, face, err_msg=name)
        np.testing.assert_array_equal(gt, t, err_msg=name)
        assert info.tolist() == [int((hit < 0).sum()), 2] and bad.sum() == 2
    t, hit, face, _ = SR.walk(sc.host, LO, S, o, d, 0.0, 100.0)
    if name == "all_free":
        assert (hit == -1).all()
    if name == "all_occupied":
        inside = (((o[:700] - LO) / S >= 0) & ((o[:700] - LO) / S < np.array(sc.shape))).all(1)
        assert inside.sum() > 100 and (t[:700][inside] == 0.0).all() and (face[:700][inside] == SR.FACE_NEAR).all()
    if name == "19x9x21":
        assert (hit >= 0).sum() > 100 and (hit < 0).sum() > 100


# ------------------------------------------------------------------ views
def _rot(yaw, pitch):
    cy, sy, cp, sp = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch)
    return np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @ np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]])


def _c2w(position, yaw=0.0, pitch=0.0):
    return np.concatenate([_rot(yaw, pitch), np.asarray(position, np.float64).reshape(3, 1)], axis=1)


def _centre(shape):
    return LO + np.asarray(shape) * S * np.array([0.5, 0.6, 0.5])


def _three_poses(shape):
    c = _centre(shape)
    return np.stack([_c2w(c), _c2w(c + [0.01, 0.02, -0.03], 0.65, -0.4), _c2w(c, 2.5, -1.2)])     # the first looks along -z exactly: axis-parallel rays


# name -> (grid, poses, W, H, focal, near, far)
VIEW_CASES = {
    "19x9x21_37x23": lambda: ("19x9x21", _three_poses((19, 9, 21)), 37, 23, 18.5, 0.0, 100.0),
    "19x9x21_64x48": lambda: ("19x9x21", _three_poses((19, 9, 21))[1:2], 64, 48, 32.0, 0.0, 100.0),
    "8x8x8_37x23": lambda: ("8x8x8", _three_poses((8, 8, 8)), 37, 23, 18.5, 0.0, 100.0),
    "70x9x40_37x23": lambda: ("70x9x40", _three_poses((70, 9, 40)), 37, 23, 18.5, 0.0, 100.0),
    "all_free": lambda: ("all_free", _three_poses((11, 9, 10)), 37, 23, 18.5, 0.0, 100.0),
    "all_occupied": lambda: ("all_occupied", _three_poses((9, 5, 10)), 37, 23, 18.5, 0.0, 100.0),
    "camera_outside": lambda: ("19x9x21", np.stack([_c2w(LO + np.array([9.5, 14.0, 40.0]) * S, 0.0, -0.2), _c2w(LO + np.array([-15.0, 6.0, 10.0]) * S, -1.4, -0.1)]),
                               37, 23, 18.5, 0.0, 100.0),
    "near_inside_the_floor": lambda: ("19x9x21", _c2w(_centre((19, 9, 21)), 0.3, -1.5)[None], 37, 23, 18.5, 4.9 * S, 100.0),
    "far_short_of_the_floor": lambda: ("19x9x21", _c2w(_centre((19, 9, 21)), 0.3, -1.5)[None], 37, 23, 18.5, 0.0, 3.0 * S),
    "nan_pose": lambda: ("19x9x21", np.stack([_c2w(_centre((19, 9, 21)), 0.3, -0.5), _c2w([np.nan, 0.0, 1.0])]), 37, 23, 18.5, 0.0, 100.0),
}


@pytest.mark.parametrize("case", list(VIEW_CASES))
def test_views_equal_the_restatement(case):
    grid, c2w, W, H, focal, near, far = VIEW_CASES[case]()
    sc = gpu_scene(grid)
    want = SR.views(sc.host, LO, S, c2w, W, H, focal, near, far)
    got = gpu_views(sc, c2w, W, H, focal, near, far)
    for k in ("hit", "rgba", "sem", "depth", "info"):
        np.testing.assert_array_equal(got[k], want[k], err_msg=f"{case} {k}")
    hit = want["hit"] >= 0
    if case == "19x9x21_37x23":
        o, d, cam0, _ = SR.view_rays(c2w, W, H, focal)
        assert cam0[18] == 0.0 and (d[0, :, 18, 0] == 0.0).all() and hit.any() and (~hit).any()      # the odd width: a column of rays with d_x exactly 0
        assert len(np.unique(want["face"][hit])) >= 3
    if case == "all_free":
        assert not hit.any() and (got["rgba"].reshape(-1, 4) == [0, 0, 0, 255]).all() and (got["depth"] == 0).all() and got["info"][0] == hit.size
    if case == "all_occupied":
        assert hit.all() and (want["face"] == SR.FACE_NEAR).all() and (got["depth"] == 0).all()
    if case == "camera_outside":
        assert hit.any() and (want["face"][hit] != SR.FACE_NEAR).all()
    if case == "near_inside_the_floor":
        assert (want["face"][hit] == SR.FACE_NEAR).sum() > 20 and (want["depth64"][want["face"] == SR.FACE_NEAR] == 4.9 * S).all()
    if case == "far_short_of_the_floor":
        assert (~hit).sum() > 100 and (want["depth64"][hit] <= 3.0 * S).all()            # the floor is 4.4 voxels below the camera
    if case == "nan_pose":
        assert got["info"].tolist() == [int((~hit).sum()), W * H] and not hit[1].any()
    # ray-mode depth, another shade table and background, no hit plane
    shade, bg = np.array([10, 255, 0, 77, 128, 200, 33], np.uint8), 0x80FF7F01
    want_r = SR.views(sc.host, LO, S, c2w, W, H, focal, near, far, ray_depth=True, shade=shade, background=bg)
    got_r = gpu_views(sc, c2w, W, H, focal, near, far, ray_depth=True, want_hit=False, shade=shade, background=bg)
    np.testing.assert_array_equal(got_r["rgba"], want_r["rgba"])
    np.testing.assert_array_equal(got_r["sem"], want_r["sem"])
    assert (np.abs(got_r["depth"].astype(np.float64) - want_r["depth"]) <= np.spacing(want_r["depth"])).all()
    if (~hit).any():
        assert (got_r["rgba"][~hit] == [0x01, 0x7F, 0xFF, 0x80]).all()


def test_no_views_and_no_rays_are_no_ops():
    sc = gpu_scene("19x9x21")
    got = gpu_views(sc, np.zeros((0, 3, 4)), 37, 23, 18.5, 0.0, 100.0)
    assert got["rgba"].size == 0 and got["info"].tolist() == [0, 0]
    t, h, f, info = gpu_cast(sc, np.zeros((0, 3)), np.zeros((0, 3)), 0.0, 1.0)
    assert t.size == 0 and info.tolist() == [0, 0]


def test_argument_errors_are_refused_before_any_launch():
    L, lib = _lib()
    sc = gpu_scene("19x9x21")
    dev = torch.device(DEV)
    W, H, P = 8, 4, 32
    m = _dev(_c2w([0.0, 0.0, 0.0])[None])
    o = _dev(np.zeros((4, 3)))
    rw, rgba = _guarded(4 * P, torch.uint8)
    dw, dep = _guarded(P, torch.float32)
    sw, sem = _guarded(P, torch.uint8)
    tw, t = _guarded(4, torch.float64)
    hw, hit = _guarded(4, torch.int32)
    fw, face = _guarded(4, torch.uint8)
    info = torch.zeros(2, dtype=torch.int64, device=DEV)

    def off(tensor, nbytes):
        p = L.DevPtr(tensor.data_ptr() + nbytes)
        p.device = tensor.device
        return p

    vox, X, Y, Z, bricks, lo, s = sc.args()
    good_scene = dict(vox=vox, X=X, Y=Y, Z=Z, bricks=bricks, lo=lo, s=s)
    good_view = dict(m=L.ptr(m), V=1, W=W, H=H, focal=4.0, near=0.0, far=10.0, mode=0, shade=_shade(), bg=0, rgba=L.ptr(rgba), dep=L.ptr(dep), sem=L.ptr(sem),
                     hit=None, info=L.ptr(info))
    good_cast = dict(o=L.ptr(o), d=L.ptr(o), n=4, near=0.0, far=10.0, t=L.ptr(t), hit=L.ptr(hit), face=L.ptr(face), info=L.ptr(info))
    nan, inf = float("nan"), float("inf")
    scene_bad = [dict(X=0), dict(Y=-1), dict(X=1024, Y=1024, Z=1024), dict(X=1 << 25), dict(vox=None), dict(bricks=None), dict(lo=None), dict(lo=_c3([nan, 0, 0])),
                 dict(s=0.0), dict(s=nan), dict(s=inf), dict(vox=off(sc.voxels, 2))]
    view_bad = [dict(V=-1), dict(W=0), dict(H=0), dict(W=16385), dict(focal=0.0), dict(focal=nan), dict(near=-1.0), dict(far=-1.0), dict(near=2.0, far=1.0),
                dict(far=inf), dict(far=nan), dict(mode=2), dict(shade=None), dict(m=None), dict(rgba=None), dict(dep=None), dict(sem=None), dict(info=None),
                dict(m=off(m, 4)), dict(rgba=off(rgba, 1)), dict(dep=off(dep, 2)), dict(info=off(info, 4))]
    cast_bad = [dict(n=-1), dict(o=None), dict(d=None), dict(t=None), dict(hit=None), dict(face=None), dict(info=None), dict(near=-0.5), dict(far=inf),
                dict(o=off(o, 4)), dict(t=off(t, 4)), dict(hit=off(hit, 2))]
    for bad in scene_bad + view_bad:
        a = dict(good_scene, **good_view)
        a.update(bad)
        with pytest.raises(L.MnfError):
            L.launch(lib.mnf_sensor_views, a["vox"], a["X"], a["Y"], a["Z"], a["bricks"], a["lo"], a["s"], a["m"], a["V"], a["W"], a["H"], a["focal"], a["near"],
                     a["far"], a["mode"], a["shade"], a["bg"], a["rgba"], a["dep"], a["sem"], a["hit"], a["info"], device=dev)
    for bad in scene_bad + cast_bad:
        a = dict(good_scene, **good_cast)
        a.update(bad)
        with pytest.raises(L.MnfError):
            L.launch(lib.mnf_sensor_cast_rays, a["vox"], a["X"], a["Y"], a["Z"], a["bricks"], a["lo"], a["s"], a["o"], a["d"], a["n"], a["near"], a["far"], a["t"],
                     a["hit"], a["face"], a["info"], device=dev)
    for shape in ((0, 1, 1), (1024, 1024, 1024)):
        assert lib.mnf_sensor_bricks_words(*shape) == -1
        with pytest.raises(L.MnfError):
            L.launch(lib.mnf_sensor_build_bricks, vox, *shape, bricks, device=dev)
    with pytest.raises(L.MnfError):
        L.launch(lib.mnf_sensor_build_bricks, None, X, Y, Z, bricks, device=dev)
    torch.cuda.synchronize()
    for w, k, what in ((rw, 4 * P, "rgba"), (dw, P, "depth"), (sw, P, "sem"), (tw, 4, "t_hit"), (hw, 4, "hit"), (fw, 4, "face")):
        _assert_guards(w, k, what)
        assert (w.cpu().numpy() == MARKS[w.dtype]).all(), f"{what} was written by a refused call"
    assert info.tolist() == [0, 0]


# ------------------------------------------------------------------ the Python surface and the stages it feeds
ROOM_AABB = np.array([-2.0, -0.2, -2.0, 2.0, 2.2, 2.0])
EYE = np.array([0.1, 1.0, -0.1])


def _room(refine=2):
    from apnrf_amd import sensor as SN
    from apnrf_amd import synthetic as S
    key = ("room", refine)
    if key not in _SCENES:
        res = [20, 12, 20]
        occ = S.make_occupancy(res, seed=4, clutter=0.02, aabb=ROOM_AABB, free_at=[EYE])
        _SCENES[key] = (SN.VoxelScene.from_occupancy(occ, ROOM_AABB, cell=0.2, refine=refine, closed=True, device=DEV), occ)
    return _SCENES[key]


def test_sample_images_from_poses_surface():
    from apnrf_amd import render as RD
    from apnrf_amd import sensor as SN
    from apnrf_amd import synthetic as S
    scene, occ = _room()
    words, lo, s = SN.occupancy_words(occ, ROOM_AABB, refine=2, closed=True)
    assert np.array_equal(scene.voxels.cpu().numpy().view(np.uint32), words) and scene.shape == (40, 24, 40)
    assert np.array_equal(scene.bricks.cpu().numpy().view(np.uint32), SR.build_bricks(words))
    sim = SN.VoxelSim(scene, 37, 23)
    assert sim.focal == 0.5 * 37 / np.tan(np.pi / 2 / 2)
    poses = S.camera_poses(EYE, 3)
    rgba, depth, sem, hit = sim.sample_images_from_poses(poses, hit=True)
    assert rgba.is_cuda and rgba.dtype == torch.uint8 and tuple(rgba.shape) == (3, 23, 37, 4) and depth.dtype == torch.float32 and sem.dtype == torch.uint8
    c2w = np.stack([RD.pose_to_c2w(p) for p in poses])[:, :3, :]
    want = SR.views(words, lo, s, c2w, 37, 23, sim.focal, 0.0, 1e3, shade=SN.DEFAULT_SHADE, background=SN.DEFAULT_BACKGROUND)
    np.testing.assert_array_equal(rgba.cpu().numpy(), want["rgba"])
    np.testing.assert_array_equal(depth.cpu().numpy(), want["depth"])
    np.testing.assert_array_equal(sem.cpu().numpy(), want["sem"])
    np.testing.assert_array_equal(hit.cpu().numpy(), want["hit"])
    assert sim.info.tolist() == [0, 0]                                                 # a closed room: every ray ends on a surface
    h_rgba, h_depth, h_sem = sim.sample_images_from_poses(poses, host=True)
    assert isinstance(h_rgba, np.ndarray) and h_rgba.dtype == np.uint8 and h_depth.dtype == np.float32 and h_sem.dtype == np.int64
    assert h_rgba[:, :, :, :3].shape == (3, 23, 37, 3) and np.array_equal(h_rgba, want["rgba"])
    cast = sim.cast_rays(np.tile(EYE, (5, 1)), np.array([[0, -1.0, 0], [1.0, 0, 0], [0, 0, -1.0], [0.3, 0.2, 0.9], [0, 1.0, 0]]))
    t, lin, face, _ = SR.walk(words, lo, s, np.tile(EYE, (5, 1)), np.array([[0, -1.0, 0], [1.0, 0, 0], [0, 0, -1.0], [0.3, 0.2, 0.9], [0, 1.0, 0]]), 0.0, 1e3)
    assert np.array_equal(cast["t_hit"].cpu().numpy(), t) and np.array_equal(cast["hit"].cpu().numpy(), lin) and np.array_equal(cast["face"].cpu().numpy(), face)
    pc = SN.VoxelScene.from_point_cloud(np.array([[0.05, 0.05, 0.05], [0.06, 0.05, 0.05], [0.35, 0.05, 0.05]]), np.array([[1, 2, 3], [4, 5, 6], [7, 8, 9]], np.uint8),
                                        np.array([5, 6, 7]), 0.1, lo=[0, 0, 0], device=DEV)
    assert pc.voxels.cpu().numpy().view(np.uint32).reshape(-1).tolist() == [0x05030201, 0xFF000000, 0xFF000000, 0x07090807]


def _captures(W=64, n=4, depth="ray"):
    from apnrf_amd import render as RD
    from apnrf_amd import sensor as SN
    from apnrf_amd import synthetic as S
    scene, _ = _room()
    sim = SN.VoxelSim(scene, W, W)
    poses = S.camera_poses(EYE, n)
    rgba, dep, sem, hit = sim.sample_images_from_poses(poses, depth=depth, hit=True)
    c2w = torch.from_numpy(np.stack([RD.pose_to_c2w(p) for p in poses])).to(DEV)
    return scene, sim, rgba, dep, sem, hit, c2w


def test_captures_line_up_with_the_datasets_rays(tmp_path):
    """Capture -> `update_data` from device tensors -> `fetch_data` in evaluation mode: origin + ray_depth * viewdir of every hit pixel lies
    in its hit voxel.  THE BOUND: the sensor forms the ray in float64 from the float64 pose; the dataset stores the pose in float32 (each
    entry within 2^-24 relative) and forms cam, the three products and two sums of a direction, its norm and the division in float32: a
    dozen roundings of 2^-24 on a direction component of size <= |cam|, then the float32 depth (2^-24 relative) and the float32 origin.
    The point therefore moves by at most 16 * 2^-24 * (depth * |cam| + |origin|) <= 16 * 2^-24 * (2 depth + 4) metres along each axis;
    the voxel is widened by that: about 1e-5 of its 0.1 m edge."""
    from apnrf_amd.dataset import Dataset
    scene, sim, rgba, dep, sem, hit, c2w = _captures()
    ds = Dataset(training=False, save_fp=str(tmp_path / "d"), device=DEV)
    with pytest.raises(ValueError):
        ds.update_data(rgba, dep, sem, c2w)                                            # the RGBA refusal stays
    ds.update_data(rgba[..., :3], dep, sem, c2w)
    assert len(ds) == 4 and ds.images.is_cuda and ds.depths.dtype == torch.float32 and ds.semantics.dtype == torch.int64 and ds._focal == float(np.float32(sim.focal))
    X, Y, Z = scene.shape
    for i in (0, 3):
        data = ds.fetch_data(i)
        np.testing.assert_array_equal(data["rgb"].cpu().numpy(), rgba[i, :, :, :3].cpu().numpy().astype(np.float32) / np.float32(255.0))   # IEEE division, as the gather's
        assert torch.equal(data["dep"], dep[i]) and torch.equal(data["sem"], sem[i].to(torch.int64))
        o = data["rays"].origins.cpu().numpy().astype(np.float64)
        v = data["rays"].viewdirs.cpu().numpy().astype(np.float64)
        z = dep[i].cpu().numpy().astype(np.float64)
        lin = hit[i].cpu().numpy().astype(np.int64)
        assert (lin >= 0).all()
        p = (o + z[..., None] * v - scene.lo) / scene.voxel_size
        cell = np.stack([lin // (Y * Z), (lin // Z) % Y, lin % Z], axis=-1).astype(np.float64)
        slack = (16 * 2.0 ** -24 * (2 * z + 4) / scene.voxel_size)[..., None]
        assert ((p >= cell - slack) & (p <= cell + 1 + slack)).all(), float(np.max(np.maximum(cell - p, p - cell - 1)))
    # host arrays go the way they always went
    ds_h = Dataset(training=False, save_fp=str(tmp_path / "h"), device=DEV)
    ds_h.update_data(rgba[..., :3].cpu().numpy(), dep.cpu().numpy(), sem.cpu().numpy().astype(np.int64), c2w.cpu().numpy())
    for a, b in ((ds.images, ds_h.images), (ds.depths, ds_h.depths), (ds.semantics, ds_h.semantics), (ds.camtoworlds, ds_h.camtoworlds)):
        assert a.dtype == b.dtype and torch.equal(a, b)
    packed = Dataset(training=False, save_fp=str(tmp_path / "p"), device=DEV, packed=True)
    packed.update_data(rgba[..., :3], dep, sem, c2w)
    assert packed.depths.dtype == torch.float16 and packed.semantics.dtype == torch.uint8 and torch.equal(packed.semantics, sem)


def test_cost_map_and_exploration_map_accept_the_captures(tmp_path):
    from apnrf_amd.dataset import Dataset
    from apnrf_amd.explore import ExplorationMap
    from apnrf_amd.planning import ScanCostMap
    scene, sim, rgba, dep, sem, hit, c2w = _captures(depth="z")
    cost = ScanCostMap(ROOM_AABB, 0.2, device=DEV)
    cost.update(dep, c2w)
    info = cost.info()
    assert info["bad_depth"] == 0 and info["drawn"] > 0 and int((cost.codes == 1).sum()) > 0 and int((cost.codes == 2).sum()) > 0
    ds = Dataset(training=False, save_fp=str(tmp_path / "d"), device=DEV)
    ds.update_data(rgba[..., :3], dep, sem, c2w)
    emap = ExplorationMap(ROOM_AABB, voxel_size=0.1, max_range=10.0, device=DEV)
    emap.insert_dataset(ds, [0, 1, 2, 3], depth_along="z")
    counts = emap.counts()
    assert counts["free"] > 1000 and counts["occupied"] > 100
    assert sim.info.tolist() == [0, 0]


def test_training_on_captures_improves_held_out_views(tmp_path):
    """End to end: 16 captured views train a small field for 300 deterministic steps; on 2 held-out captures `evaluate_views` must report a
    strictly lower depth MSE and a strictly higher PSNR than for the same field and estimator before training.  Depth is captured along
    the ray ("ray"), what the field's rendered depth is.  A comparison against the untrained field, not a threshold.  On one MI355X:
    depth MSE 3.77729 -> 0.15558, PSNR 3.606 -> 15.585 (the untrained field with its empty grid renders the white background)."""
    from apnrf_amd import nerfacc as NA
    from apnrf_amd import render as RD
    from apnrf_amd import scenes as SC
    from apnrf_amd import sensor as SN
    from apnrf_amd import synthetic as S
    from apnrf_amd.dataset import Dataset
    from apnrf_amd.ngp import NGPRadianceField
    from apnrf_amd.optim import FusedAdam
    cfg = SC.make_scene(log2_hashmap_size=14, n_poses=1)                               # the field's shape: 128 x 2, 29 classes, a 2^14 table
    scene, _ = _room()
    sim = SN.VoxelSim(scene, 64, 64)
    poses = S.camera_poses(EYE, 18)
    held = [4, 13]
    train = [i for i in range(18) if i not in held]
    c2w = torch.from_numpy(np.stack([RD.pose_to_c2w(p) for p in poses])).to(DEV)
    rgba, dep, sem = sim.sample_images_from_poses(poses, depth="ray")
    assert sim.info.tolist() == [0, 0]
    ds = Dataset(training=True, save_fp=str(tmp_path / "t"), num_rays=1024, device=DEV)
    ds.update_data(rgba[train][..., :3], dep[train], sem[train], c2w[train])
    ev = Dataset(training=False, save_fp=str(tmp_path / "e"), device=DEV)
    ev.update_data(rgba[held][..., :3], dep[held], sem[held], c2w[held])
    aabb = torch.from_numpy(ROOM_AABB.astype(np.float32))
    field = NGPRadianceField(aabb=aabb, neurons=cfg["neurons"], layers=cfg["layers"], num_semantic_classes=cfg["C"], log2_hashmap_size=cfg["log2_hashmap_size"],
                             seed=9).to(DEV)
    est = NA.OccGridEstimator(aabb, resolution=[20, 12, 20], levels=1).to(DEV)
    opt = FusedAdam(field.parameters(), lr=2e-3, eps=1e-15).bind_field(field)
    before = RD.evaluate_views(field.eval(), est.eval(), ev, [0, 1], **SC.RENDER_KW)["mean"]
    rng_state = torch.random.get_rng_state()
    torch.manual_seed(1234)
    for step in range(300):
        b = ds[0]
        RD.train_step(field, est, opt, b["rays"], b["pixels"], b["dep"], b["sem"], b["color_bkgd"], step=step, occ_thre=1e-2, deterministic=True, **SC.RENDER_KW)
    torch.random.set_rng_state(rng_state)
    after = RD.evaluate_views(field.eval(), est.eval(), ev, [0, 1], **SC.RENDER_KW)["mean"]
    print(f"held-out views before training: depth MSE {before['depth_mse']:.5f}, PSNR {before['psnr']:.3f}; after 300 steps: depth MSE "
          f"{after['depth_mse']:.5f}, PSNR {after['psnr']:.3f}")
    assert after["depth_mse"] < before["depth_mse"] and after["psnr"] > before["psnr"]
