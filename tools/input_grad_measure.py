"""Measurement of the input-gradient kernel: one batch of 262 144 samples of the bench model (128 x 2, 29 classes, 2^19-entry
tables), positions uniform in the box (no two neighbouring samples share a fine cell: the gathers' worst case), one process, after warm-up.
`NGPRadianceField.forward` + backward with positions and directions requiring gradients; time per launch from the library's hipEvent pairs
(`mnf_profile_begin/end`) for "field_input_grad" beside "field_train_forward", "dgrad", "wgrad" and "hash_scatter" of the same batch.

    python tools/input_grad_measure.py [--n 262144] [--reps 10] [--out FILE]
"""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import apnrf_amd  # noqa: E402
from apnrf_amd import scenes as SC  # noqa: E402

DEV = "cuda:0"
LABELS = ("field_train_forward", "dgrad", "wgrad", "hash_scatter", "field_input_grad")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=262144)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lib = apnrf_amd.load_library()
    scene = SC.make_scene()
    field = SC.hip_field(scene, DEV).train()
    rng = np.random.default_rng(0)
    box = scene["aabb"]
    pos = torch.from_numpy((rng.random((a.n, 3)) * (box[3:] - box[:3]) * 0.98 + box[:3] + 0.01 * (box[3:] - box[:3])).astype(np.float32)).to(DEV)
    d = rng.normal(size=(a.n, 3)).astype(np.float32)
    d = torch.from_numpy(d / np.linalg.norm(d, axis=-1, keepdims=True)).to(DEV)
    g = [torch.from_numpy((rng.normal(size=(a.n, k)) * s).astype(np.float32)).to(DEV) for k, s in ((3, 1e-3), (1, 1e-5), (scene["C"], 1e-3))]

    def step(inputs):
        p, q = pos.clone().requires_grad_(inputs), d.clone().requires_grad_(inputs)
        torch.autograd.backward(list(field(p, q)), g)
        field.zero_grad()

    lines = []
    for inputs in (False, True):
        for _ in range(3):
            step(inputs)
        torch.cuda.synchronize()
        lib.mnf_profile_begin()
        for _ in range(a.reps):
            step(inputs)
        torch.cuda.synchronize()
        lib.mnf_profile_end(None, None)
        parts = []
        for label in LABELS:
            ms, cnt = ctypes.c_double(), ctypes.c_int64()
            lib.mnf_profile_query(label.encode(), ctypes.byref(ms), ctypes.byref(cnt))
            parts.append(f"{label} {1e3 * ms.value / max(cnt.value, 1):.1f} us x {cnt.value}")
        lines.append(f"n = {a.n}, input gradients {'on ' if inputs else 'off'}: " + ", ".join(parts))
        print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
