"""CPU-side checks of the held-out view evaluation (`mnf_eval_views`, csrc/eval.hip; render.eval_metrics / evaluate_views): the two
symbols are declared, exported and bound; every argument error is refused with MNF_ERR_INVALID before anything touches a device; and
`miou_from_confusion` gives the hand-worked value of a small matrix."""
import ctypes
import os
import re

import numpy as np
import pytest

import apnrf_amd
from apnrf_amd import _lib as L

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("mnf_eval_views_workspace_bytes", "mnf_eval_views")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as G
    G.build()
    return apnrf_amd.load_library()


def test_eval_symbols_declared_exported_and_bound(lib):
    header = open(os.path.join(REPO, "include", "mi355nerf.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    raw = ctypes.CDLL(L.lib_path())
    for s in SYMBOLS:
        assert re.search(r"\b" + s + r"\s*\(", code), f"{s} is not declared in include/mi355nerf.h"
        assert hasattr(raw, s), f"{s} is not exported"
        assert s in L.SIGNATURES
    assert L.SIGNATURES["mnf_eval_views_workspace_bytes"][0] is ctypes.c_int64
    assert len(L.SIGNATURES["mnf_eval_views"][1]) == 20                      # 19 arguments + the stream
    assert header.count("typedef struct {") == 5                             # plain arguments: the entry point adds no struct
    assert "pipeline.py:550-613" in header and ":1011" in header             # names what it replaces


def test_eval_workspace_bytes(lib):
    one = lib.mnf_eval_views_workspace_bytes(1, 800 * 800, 29)
    assert one > 0 and one % 8 == 0
    assert lib.mnf_eval_views_workspace_bytes(4, 800 * 800, 29) == 4 * one   # a view's split does not depend on the other views
    assert lib.mnf_eval_views_workspace_bytes(0, 800 * 800, 29) == 0
    assert 0 < lib.mnf_eval_views_workspace_bytes(1, 1, 29) <= one
    for bad in [(1, 0, 29), (1, 16, 0), (-1, 16, 29)]:
        assert lib.mnf_eval_views_workspace_bytes(*bad) == 0


def _call(lib, **over):
    """mnf_eval_views with plausible (never dereferenced) pointers; `over` replaces arguments by name."""
    V, P, C = 2, 64, 29
    a = dict(rgb=0x1000, depth=0x2000, sem=0x3000, n_views=V, n_pix=P, n_classes=C, gt_images=0x4000, gt_depths=0x5000, depth_is_f16=0,
             gt_semantics=0x6000, sem_is_u8=0, pixels_per_image=P, image_ids=0x7000, pix_idx=None, metrics=0x8000, confusion=None,
             pred_labels=None, workspace=0x9000, workspace_bytes=None, stream=None)
    a.update(over)
    if a["workspace_bytes"] is None:
        a["workspace_bytes"] = lib.mnf_eval_views_workspace_bytes(a["n_views"], a["n_pix"], a["n_classes"])
    rc = lib.mnf_eval_views(*a.values())
    return rc, lib.mnf_last_error().decode()


@pytest.mark.parametrize("name", ["rgb", "depth", "sem", "gt_images", "gt_depths", "gt_semantics", "image_ids", "metrics", "workspace"])
def test_eval_refuses_null_required_pointer(lib, name):
    rc, msg = _call(lib, **{name: None})
    assert rc == -1 and name in msg, (rc, msg)


def test_eval_refuses_bad_sizes(lib):
    rc, msg = _call(lib, n_classes=0, workspace_bytes=1 << 20)
    assert rc == -1 and "n_classes" in msg, (rc, msg)
    rc, msg = _call(lib, n_classes=-3, workspace_bytes=1 << 20)
    assert rc == -1 and "n_classes" in msg, (rc, msg)
    rc, msg = _call(lib, n_pix=0, workspace_bytes=1 << 20)
    assert rc == -1 and "n_pix" in msg, (rc, msg)
    rc, msg = _call(lib, n_pix=-5, workspace_bytes=1 << 20)
    assert rc == -1 and "n_pix" in msg, (rc, msg)


def test_eval_refuses_small_workspace(lib):
    need = lib.mnf_eval_views_workspace_bytes(2, 64, 29)
    rc, msg = _call(lib, workspace_bytes=need - 1)
    assert rc == -1 and "workspace" in msg, (rc, msg)
    rc, msg = _call(lib, workspace_bytes=0)
    assert rc == -1 and "workspace" in msg, (rc, msg)


def test_eval_refuses_pred_labels_above_256_classes(lib):
    rc, msg = _call(lib, n_classes=257, pred_labels=0xA000)
    assert rc == -1 and "pred_labels" in msg, (rc, msg)


def test_eval_zero_views_is_ok(lib):
    rc, _ = _call(lib, n_views=0, rgb=None, depth=None, sem=None, metrics=None, workspace=None, workspace_bytes=0)
    assert rc == 0


def test_miou_from_confusion_hand_worked():
    from apnrf_amd.render import miou_from_confusion
    # rows: ground truth, columns: prediction.  Class 3 occurs in neither; class 2 only as a (wrong) prediction.
    m = np.array([[5, 1, 0, 0],
                  [2, 3, 1, 0],
                  [0, 0, 0, 0],
                  [0, 0, 0, 0]], dtype=np.int64)
    # class 0: TP 5, FP 2, FN 1 -> 5/8;  class 1: TP 3, FP 1, FN 3 -> 3/7;  class 2: TP 0, FP 1, FN 0 -> 0;  class 3: absent
    want = (5.0 / 8.0 + 3.0 / 7.0 + 0.0) / 3.0
    assert miou_from_confusion(m) == pytest.approx(want, rel=1e-15)
    import torch
    assert miou_from_confusion(torch.from_numpy(m)) == pytest.approx(want, rel=1e-15)
    assert miou_from_confusion(np.diag([4, 0, 9])) == 1.0                   # the empty class does not pull the mean down
    assert np.isnan(miou_from_confusion(np.zeros((3, 3), np.int64)))
