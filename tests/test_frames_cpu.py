"""CPU-side checks of the 8-bit frame conversion (`mnf_frames_views`, csrc/frames.hip; render.frames_from_renders / render_frames):
known answers of the numpy restatement the GPU tests are held to (tests/frames_ref.py), the two precision rules shown on the inputs
that tell them apart, and the entry point's symbol and refusals, which need the built library but no device."""
import ctypes
import os
import re

import numpy as np
import pytest

import apnrf_amd
import frames_ref as FR
from apnrf_amd import _lib as L

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")


def test_sat8_known_answers():
    x = np.array([0.5, 1.5, 2.5, 254.5, 255.5, 300.0, INF, -3.0, -INF, NAN, 0.0, 255.0, 127.49999, 127.50001])
    want = [0, 2, 2, 254, 255, 255, 255, 0, 0, 0, 0, 255, 127, 128]
    assert FR.sat8(x).tolist() == want
    assert FR.sat8(x.astype(np.float32)[:10]).tolist() == want[:10]
    assert FR.sat8(x).dtype == np.uint8


def test_plane_known_answers():
    # 0.5 / 255 * 255 and friends: the planes apply sat8 to the reference's own products
    assert FR.occ8(np.float32([0.0, 1.0, 1.2, -0.1, NAN, INF, -INF, 0.5])).tolist() == [0, 255, 255, 0, 0, 255, 0, 128]     # 127.5 -> 128 (even)
    assert FR.rgb8(np.float32([0.0, 1.0, 1.2, -0.1, NAN, INF, -INF, 0.5])).tolist() == [0, 255, 255, 0, 0, 255, 0, 128]
    assert FR.dep8(np.float32([0.0, 0.5, 1.5, 0.02, 10.0, 10.5, 14.0, -1.0, NAN, INF, -INF])).tolist() == [0, 12, 38, 0, 250, 255, 255, 0, 0, 255, 0]
    assert FR.dep8(np.float32([0.0, 5.0, 10.0, 12.0, -1.0, NAN, INF, -INF, 0.25]), FR.DEPTH_VIEWER).tolist() == [0, 128, 255, 255, 0, 0, 255, 0, 6]
    # a depth map of the caller's: clip(d * 2 / 4, 0, 3) * 10
    assert FR.dep8(np.float32([1.0, 5.0, 100.0]), (2.0, 4.0, 3.0, 10.0)).tolist() == [5, 25, 30]


def test_argmax_ties_and_nan():
    sem = np.float32([[1.0, 4.0, 4.0, 0.0],          # tie: the first index
                      [2.5, 2.5, 2.5, 2.5],
                      [1.0, 9.0, NAN, 3.0],          # a NaN logit wins
                      [NAN, 9.0, NAN, 3.0],          # the first NaN
                      [-INF, -INF, -INF, -INF]])
    assert FR.label_map(sem).tolist() == [1, 0, 2, 0, 0]
    pal = np.array([[10, 20, 30], [40, 50, 60], [70, 80, 90], [1, 2, 3]], np.uint8)
    z = np.zeros(5, np.float32)
    f = FR.frames(np.zeros((5, 3), np.float32), z, z, sem, pal, channel_order="rgb")
    assert f["sem"].tolist() == [[40, 50, 60], [10, 20, 30], [70, 80, 90], [10, 20, 30], [10, 20, 30]]
    b = FR.frames(np.float32([[0.0, 0.5, 1.0]] * 5), z, z, sem, pal, channel_order="bgr")
    assert b["sem"].tolist() == [[60, 50, 40], [30, 20, 10], [90, 80, 70], [30, 20, 10], [30, 20, 10]]
    assert b["rgb"][0].tolist() == [255, 128, 0]


def test_depth_is_float64_and_rgb_is_float32():
    """The precision rules are not a nicety: next to the k + 0.5 boundaries the float32 form of the depth expression and the float64 form
    of the colour expression give other bytes than the reference's.  A kernel "simplified" to one precision fails the GPU test on these."""
    d = FR.depth_boundary_set()
    assert d.dtype == np.float32 and d.shape == (510,)
    n_dep = int((FR.depth_f32_form(d) != FR.dep8(d)).sum())
    x = FR.unit_boundary_set()
    n_rgb = int((FR.rgb_f64_form(x) != FR.rgb8(x)).sum())
    print(f"depth: float32 form differs on {n_dep} of {d.size}; rgb: float64 form differs on {n_rgb} of {x.size}")
    assert n_dep > 0 and n_rgb > 0
    # occ8 is the float64 product: on the same inputs it is the form the colour plane must NOT take
    assert (FR.occ8(x) == FR.rgb_f64_form(x)).all()
    # np.float32(float64(x) * 255) is x * 255 rounded once to float32: the kernel's single-precision product
    v = np.random.default_rng(0).uniform(-0.1, 1.2, 200000).astype(np.float32)
    assert (np.float32(v.astype(np.float64) * 255) == v * np.float32(255)).all()


# ------------------------------------------------------------------ the entry point, without a device
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as G
    G.build()
    return apnrf_amd.load_library()


def test_frames_symbol_declared_exported_and_bound(lib):
    header = open(os.path.join(REPO, "include", "mi355nerf.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"\bmnf_frames_views\s*\(", code), "mnf_frames_views is not declared in include/mi355nerf.h"
    assert hasattr(ctypes.CDLL(L.lib_path()), "mnf_frames_views"), "mnf_frames_views is not exported"
    res, args = L.SIGNATURES["mnf_frames_views"]
    assert res is ctypes.c_int32 and len(args) == 20                         # 19 arguments + the stream
    assert args[9:13] == [ctypes.c_double] * 4                               # the depth mapping crosses the boundary in double
    assert header.count("typedef struct {") == 5                             # plain arguments: no options struct
    assert "pipeline.py:976-1023" in header


def _call(lib, **over):
    """mnf_frames_views with plausible (never dereferenced) pointers; `over` replaces arguments by name."""
    a = dict(rgb=0x1000, depth=0x2000, acc=0x3000, sem=0x4000, n_views=2, n_pix=64, n_classes=29, palette=0x5000, palette_entries=40,
             depth_mul=25.0, depth_div=1.0, depth_clip_hi=255.0, depth_gain=1.0, bgr=1, rgb8=0x6000, dep8=0x7000, occ8=0x8000, sem8=0x9000,
             labels=0xA000, stream=None)
    assert not set(over) - set(a)
    a.update(over)
    rc = lib.mnf_frames_views(*a.values())
    return rc, lib.mnf_last_error().decode()


@pytest.mark.parametrize("over, word", [
    (dict(n_views=-1), "n_views"), (dict(n_pix=0), "n_pix"), (dict(n_pix=-7), "n_pix"), (dict(n_classes=0), "n_classes"),
    (dict(n_classes=-2), "n_classes"), (dict(palette_entries=-1), "palette_entries"),
    (dict(rgb=None), "rgb"), (dict(depth=None), "depth"), (dict(acc=None), "acc"), (dict(sem=None), "sem"), (dict(palette=None), "palette"),
    (dict(sem=None, sem8=None), "sem"), (dict(palette=None, sem8=None), "palette"),       # the label plane alone still needs both
    (dict(palette_entries=28), "palette_entries"),
    (dict(n_classes=257, palette_entries=300), "labels"),
    (dict(depth_div=0.0), "depth_div"), (dict(depth_div=-0.0), "depth_div"), (dict(depth_mul=NAN), "finite"), (dict(depth_div=INF), "finite"),
    (dict(depth_clip_hi=-INF), "finite"), (dict(depth_gain=NAN), "finite"),
    (dict(n_views=65536), "65535"),
])
def test_frames_refuses_bad_argument(lib, over, word):
    rc, msg = _call(lib, **over)
    assert rc == -1 and word in msg, (rc, msg)


def test_frames_unsupported_class_count(lib):
    rc, msg = _call(lib, n_classes=10240, palette_entries=10240, labels=None)
    assert rc == -3 and "n_classes" in msg, (rc, msg)


def test_frames_accepts_zero_views_and_nothing_to_do(lib):
    rc, msg = _call(lib, n_views=0, rgb=None, depth=None, acc=None, sem=None, palette=None, rgb8=None, dep8=None, occ8=None, sem8=None, labels=None,
                    palette_entries=0)
    assert rc == 0, msg
    rc, msg = _call(lib, n_views=0)
    assert rc == 0, msg
    # every output skipped: sem and palette may then be null, and nothing is launched
    rc, msg = _call(lib, sem=None, palette=None, palette_entries=0, rgb8=None, dep8=None, occ8=None, sem8=None, labels=None)
    assert rc == 0, msg


def test_python_surface_refuses_before_touching_a_device():
    import torch
    from apnrf_amd import render as RD
    assert RD.FRAME_DEPTH_PIPELINE == (25.0, 1.0, 255.0, 1.0) and RD.FRAME_DEPTH_VIEWER == (1.0, 10.0, 1.0, 255.0)
    assert RD.FRAME_DEPTH_PIPELINE == FR.DEPTH_PIPELINE and RD.FRAME_DEPTH_VIEWER == FR.DEPTH_VIEWER
    z = torch.zeros(1, 4, 3)
    with pytest.raises(L.MnfError, match="GPU tensors only"):
        RD.frames_from_renders(z, z[..., 0], z[..., 0], z, np.zeros((3, 3), np.uint8))
