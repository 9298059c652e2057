"""One table-gradient scatter (csrc/scatter.hip, compiled once) serves field handles of both matrix-core operand types in one process: the fp16 and the
bf16 backward (csrc/train.hip, one translation unit each) hand it their own feature gradients, workspace regions, list cursors and fixed-point buffers.
Deterministic mode is bit-reproducible, so interleaved calls on two handles must give each handle exactly what it gives alone.

Scene and batch of test_deterministic_training_is_bitwise_reproducible (tests/test_gpu_round3.py)."""
import pytest
import torch

import helpers as H
from test_gpu_round3 import _train_batch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def test_one_scatter_unit_serves_fp16_and_bf16_handles_in_one_process():
    from apnrf_amd import render as RD
    sc = H.make_scene("102344250", n_poses=40, log2_hashmap_size=17)
    o, d, pix, dep, lab = (t.to(DEV) for t in _train_batch(sc, 3, 24, 24, 0))

    def grads_of(hip, est):
        RD.fused_forward_backward(hip, est, RD.Rays(o, d), pix, dep, lab, None, stratified=False, deterministic=True, **H.RENDER_KW)
        return [m.params.grad.clone() for m in (hip.mlp_base, hip.mlp_head, hip.mlp_sem)]

    def handle(bf16):
        hip, est = H.hip_field(sc, mfma_bf16=bf16), H.hip_estimator(sc)
        hip.train()
        return hip, est

    alone = {bf16: grads_of(*handle(bf16)) for bf16 in (False, True)}      # a fresh handle of each type that runs alone
    pair = {bf16: handle(bf16) for bf16 in (False, True)}
    runs = {False: [], True: []}
    for bf16 in (False, True, False, True):
        runs[bf16].append(grads_of(*pair[bf16]))
    for bf16 in (False, True):
        first, second = runs[bf16]
        for a, b, c in zip(first, second, alone[bf16]):
            assert torch.equal(a, b)                                       # bit-identical from call to call, with the other type's backward in between
            assert torch.equal(a, c)                                       # ... and to the handle that ran alone
    # on the host: not on zeros, and not one handle answering for both (mlp_base = base MLP weights, then the hash table)
    n_table = pair[False][0]._table_entries() * 4
    table = {bf16: runs[bf16][0][0][-n_table:].cpu() for bf16 in (False, True)}
    for bf16 in (False, True):
        mlp = runs[bf16][0][0][:-n_table].cpu()
        assert float(mlp.norm()) > 0.0 and float(table[bf16].norm()) > 0.0
        assert all(float(g.cpu().norm()) > 0.0 for g in runs[bf16][0][1:])
    assert not torch.equal(table[False], table[True])
