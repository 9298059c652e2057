"""The oracle's output rounding (`OracleField(..., output_rounding=...)`) independent of the operand precision: the product's
`output_fp16` flag is honoured in the bf16 build too, so the oracle must express "bf16 operands, fp16 hand-over" (mfma_bf16=1,
output_fp16=1) as well as the tcnn mode.  CPU only."""
import numpy as np
import pytest
import torch

import helpers as H


def _oracle(sc, precision, **kw):
    from oracle.field import FieldConfig, OracleField
    cfg = FieldConfig(aabb=tuple(float(x) for x in sc["aabb"]), neurons=sc["neurons"], layers=sc["layers"], num_semantic_classes=sc["C"],
                      log2_hashmap_size=sc["log2_hashmap_size"])
    return OracleField(cfg, sc["params"], precision, False, **kw)


@pytest.fixture(scope="module")
def case():
    sc = H.make_scene(neurons=64, layers=2, C=17, log2_hashmap_size=12, head_gain=4.0)
    rng = np.random.default_rng(5)
    n = 777
    a = sc["aabb"]
    pos = torch.from_numpy((rng.random((n, 3)) * (a[3:] - a[:3]) * 1.1 + a[:3] - 0.05 * (a[3:] - a[:3])).astype(np.float32))
    d = rng.normal(size=(n, 3)).astype(np.float32)
    d = torch.from_numpy(d / np.linalg.norm(d, axis=-1, keepdims=True))
    return sc, pos, d


def _run(orc, pos, d):
    with torch.no_grad():
        rgb, sigma, sem = orc(pos, d)
        dens = orc.query_density(pos)
    return rgb, sigma, sem, dens


def _raw_outputs(orc, pos, d):
    """the three networks' outputs before any activation: the values the hand-over rounds"""
    x = (pos - orc.aabb[:3]) / (orc.aabb[3:] - orc.aabb[:3])
    with torch.no_grad():
        base = orc._mlp(orc.hash_encode(x), orc.w_base)
        geo = base[:, 1:1 + orc.cfg.geo_feat_dim]
        one = torch.ones(geo.shape[0], 1)
        head = orc._mlp(torch.cat([orc.sh4((d + 1.0) / 2.0), geo, one], -1), orc.w_head)
        sem = orc._mlp(torch.cat([geo, one], -1), orc.w_sem)
    return base, head, sem


def test_f16_with_output_rounding_is_the_tcnn_mode(case):
    sc, pos, d = case
    a, b = _run(_oracle(sc, "f16", output_rounding=True), pos, d), _run(_oracle(sc, "tcnn"), pos, d)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_bf16_with_output_rounding_rounds_the_bf16_network_to_fp16(case):
    sc, pos, d = case
    plain, rounded = _oracle(sc, "bf16"), _oracle(sc, "bf16", output_rounding=True)
    p_raw, r_raw = _raw_outputs(plain, pos, d), _raw_outputs(rounded, pos, d)
    # the base network's outputs: fp16 values, and exactly the fp16 rounding of the unrounded bf16 network's
    assert torch.equal(r_raw[0], p_raw[0].half().float())
    # the heads see the rounded geometry features, so only their grain is checked: every output of the three networks is an fp16 value
    for t in r_raw:
        assert torch.equal(t, t.half().float())
    # and NOT a bf16 value everywhere (what a bf16 hand-over would give): the rounding is fp16's 11 bits, not bf16's 8
    assert not torch.equal(r_raw[2], r_raw[2].bfloat16().float())
    rgb, sigma, sem, dens = _run(rounded, pos, d)
    p_rgb, p_sigma, p_sem, _ = _run(plain, pos, d)
    assert torch.equal(sem, r_raw[2][:, :sc["C"]])
    assert torch.equal(dens, sigma)
    inside = p_sigma[:, 0] > 0
    assert torch.equal(inside, sigma[:, 0] > 0) and 0 < int(inside.sum()) < inside.numel()
    # density = exp(logit - 1): half an fp16 ulp of the logit (2^-11 relative) moves log(density) by at most that much
    logit = p_raw[0][:, 0]
    dlog = (torch.log(sigma[:, 0].double()) - torch.log(p_sigma[:, 0].double())).abs()
    assert bool((dlog[inside] <= 2 ** -11 * 1.01 * logit[inside].abs().double() + 1e-12).all())
    assert not torch.equal(sem, p_sem) and float((sem - p_sem).abs().max()) < 5e-2
    assert float((rgb - p_rgb).abs().max()) < 5e-2


def test_default_output_rounding_follows_the_precision(case):
    sc, pos, d = case
    for prec, rounds in (("f16", False), ("bf16", False), ("f32", False), ("tcnn", True)):
        default = _oracle(sc, prec)
        assert default.output_rounding is rounds, prec
        explicit = _oracle(sc, prec, output_rounding=rounds)
        for x, y in zip(_run(default, pos, d), _run(explicit, pos, d)):
            assert torch.equal(x, y), prec
    # the unrounded modes really hand over values that are not all fp16
    sem = _run(_oracle(sc, "f16"), pos, d)[2]
    assert not torch.equal(sem, sem.half().float())
    # output_rounding=False under "tcnn" is the f16 mode
    for x, y in zip(_run(_oracle(sc, "tcnn", output_rounding=False), pos, d), _run(_oracle(sc, "f16"), pos, d)):
        assert torch.equal(x, y)
