"""Holds tests/vanilla_ref.py, the float64 restatement that tests/test_gpu_vanilla.py compares csrc/vanilla.hip with, to the definition:
against the golden-anchored oracle (oracle/vanilla.py, which tests/test_oracle_golden.py pins to the reference's recorded outputs), against
a float32 torch.nn evaluation of the product's own parameter tree on the skip shapes (concat order, parameter names), and checks that the
case table is neither vacuous (ReLUs on both sides, no dead gradient) nor short of a launch route.  CPU only."""
import functools

import numpy as np
import pytest
import torch

import vanilla_ref as VR
from oracle import vanilla as V


@functools.lru_cache(maxsize=None)
def _reference(case):
    name, n, pos_range = case
    cfg, _, seed = VR.SHAPES[name]
    c = VR.make_case(cfg, n, seed, pos_range)
    rgb, sigma, grads = VR.evaluate(c["sd"], cfg, c["x"], c["d"], c["g_rgb"], c["g_sigma"])
    pre = VR.forward({k: v.double() for k, v in c["sd"].items()}, cfg, c["x"], c["d"])[3]
    return c, rgb, sigma, grads, pre


def test_float64_forward_matches_golden_anchored_oracle(golden):
    g = golden("vanilla")
    sd = {k[3:]: g[k] for k in g.files if k.startswith("sd.")}
    cfg = dict(net_depth=2, net_width=64, skip_layer=None, net_depth_condition=1, net_width_condition=64)
    assert {k: tuple(v.shape) for k, v in sd.items() if k.startswith("mlp.")} == VR.param_shapes(cfg)
    # the bars of tests/test_oracle_golden.py::test_vanilla_field_matches_reference
    np.testing.assert_allclose(VR.encode(torch.from_numpy(g["posenc_in"]), 10).numpy(), g["posenc_out"], rtol=1e-5, atol=1e-5)
    o, d, e = g["rays_o"], g["rays_d"], g["t_edges"]
    mid = ((e[:-1] + e[1:]) / 2.0).astype(np.float32)
    pos = (o[:, None, :] + d[:, None, :] * mid[None, :, None]).astype(np.float32)[::16]            # every 16th ray: 256 rays x 32 samples
    dirs = np.ascontiguousarray(np.broadcast_to(d[::16, None, :], pos.shape))
    want_rgb, want_sigma = V.VanillaField(sd).forward(pos, dirs)
    n = pos.shape[0] * pos.shape[1]
    zeros = torch.zeros(n, 3)
    rgb, sigma, _ = VR.evaluate({k: torch.from_numpy(v) for k, v in sd.items()}, cfg, torch.from_numpy(pos).reshape(-1, 3),
                                torch.from_numpy(dirs).reshape(-1, 3), zeros, zeros[:, 0])
    np.testing.assert_allclose(rgb.numpy().reshape(want_rgb.shape), want_rgb, rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(sigma.numpy().reshape(want_sigma.shape[:-1]), want_sigma[..., 0], rtol=1e-4, atol=1e-5)
    assert (want_sigma > 0).any()


SKIP_CASES = [c for c in VR.CASES if VR.SHAPES[c[0]][0]["skip_layer"] is not None and c[1] <= 1013]


@pytest.mark.parametrize("case", SKIP_CASES, ids=VR.case_id)
def test_float64_matches_fp32_nn_tree_on_skip_shapes(case):
    """The product's module only holds the `nn.Linear` tree (constructing it loads no library): evaluated with plain float32 torch ops, as
    tests/test_gpu_parity.py::test_vanilla_field_general_shapes_match_cpu_autograd does, it agrees with `evaluate(float64)` in values and in
    every gradient, with that test's bars."""
    from apnrf_amd.mlp import VanillaNeRFRadianceField
    cfg = VR.SHAPES[case[0]][0]
    c, r_rgb, r_sigma, r_grads, _ = _reference(case)
    field = VanillaNeRFRadianceField(**cfg)
    res = field.load_state_dict(c["sd"], strict=False)                # the encoders' `scales` buffers are not parameters
    assert set(res.missing_keys) == {"posi_encoder.scales", "view_encoder.scales"} and not res.unexpected_keys
    assert [k for k, _ in field.named_parameters()] == list(VR.param_shapes(cfg))
    m = field.mlp

    def enc(v, deg):
        xb = (v[:, None, :] * torch.tensor([2.0 ** i for i in range(deg)])[:, None]).reshape(v.shape[0], -1)
        return torch.cat([v, torch.sin(torch.cat([xb, xb + 0.5 * np.pi], -1))], -1)

    e = enc(c["x"], 10)
    h = e
    for i, layer in enumerate(m.base.hidden_layers):
        h = torch.relu(layer(h))
        if cfg["skip_layer"] is not None and i % cfg["skip_layer"] == 0 and i > 0:
            h = torch.cat([h, e], -1)
    raw_sigma = m.sigma_layer.output_layer(h)
    z = torch.cat([m.bottleneck_layer.output_layer(h), enc(c["d"], 4)], -1)
    for layer in m.rgb_layer.hidden_layers:
        z = torch.relu(layer(z))
    rgb, sigma = torch.sigmoid(m.rgb_layer.output_layer(z)), torch.relu(raw_sigma)[:, 0]
    torch.autograd.backward([rgb, sigma], [c["g_rgb"], c["g_sigma"]])
    np.testing.assert_allclose(rgb.detach().numpy(), r_rgb.numpy(), atol=2e-6, rtol=1e-5)
    np.testing.assert_allclose(sigma.detach().numpy(), r_sigma.numpy(), atol=2e-6, rtol=1e-5)
    for name, p in field.named_parameters():
        want = r_grads[name].numpy()
        np.testing.assert_allclose(p.grad.numpy(), want, atol=2e-5 * float(np.abs(want).max()) + 1e-9, rtol=1e-4, err_msg=name)


@pytest.mark.parametrize("case", VR.CASES, ids=VR.case_id)
def test_case_is_not_vacuous(case):
    """From the float64 reference alone: the sigma ReLU is on for a share of the samples in [0.1, 0.9], no parameter tensor has an all-zero
    gradient, and every hidden layer has a unit that is active and a unit that is inactive on some sample.  One sample cannot have a share
    strictly between 0 and 1: for n = 1 the share is taken over the shape's samples pooled (the sample counts of a shape share their
    parameters), and the single sample must itself have sigma > 0, or the sigma layer's gradient would be zero."""
    name, n, pos_range = case
    c, _, sigma, grads, pre = _reference(case)
    if n == 1:
        pooled = torch.cat([_reference(k)[2] for k in VR.CASES if k[0] == name])
        assert sigma.item() > 0
        assert all(torch.equal(_reference(k)[0]["sd"][p], c["sd"][p]) for k in VR.CASES if k[0] == name for p in c["sd"])
    else:
        pooled = sigma
    share = (pooled > 0).double().mean().item()
    assert 0.1 <= share <= 0.9, share
    for k, g in grads.items():
        assert g.abs().max().item() > 0, k
    assert len(pre) == VR.SHAPES[name][0]["net_depth"] + VR.SHAPES[name][0]["net_depth_condition"]
    for i, z in enumerate(pre):
        assert (z > 0).any() and (z < 0).any(), i
        assert z.abs().min().item() > VR.RELU_MARGIN, i
    for t in (c["x"], c["d"], c["g_rgb"], c["g_sigma"]):
        assert t.dtype == torch.float32 and t.shape[0] == n
    assert c["x"].abs().max().item() <= pos_range and (n < 31 or c["x"].abs().max().item() > 0.8 * pos_range)


def test_route_coverage():
    """The waves and trips the case table was built for, re-derived by `launch_shape` (which restates the host arithmetic of csrc/vanilla.hip)."""
    shapes = {c: VR.launch_shape(VR.SHAPES[c[0]][0], c[1]) for c in VR.CASES}
    by_name = {c[0]: s for c, s in shapes.items()}
    want = {"default": (1, 2, 264), "skip-last": (2, 3, 192), "widest": (1, 1, 520), "narrow-net": (1, 1, 512), "odd-tiles": (3, 4, 104),
            "deepest": (4, 4, 40), "second-trip": (1, 1, 328)}
    assert {k: (s["fwd_waves"], s["bwd_waves"], s["buf_rows"]) for k, s in by_name.items()} == want
    assert {s["fwd_waves"] for s in shapes.values()} == {1, 2, 3, 4} and {s["bwd_waves"] for s in shapes.values()} == {1, 2, 3, 4}
    assert any(s["fwd_second_trip"] for s in shapes.values()) and any(s["bwd_second_trip"] for s in shapes.values())
    st = shapes[("second-trip", 32805, 1.5)]
    assert (st["tiles"], st["fwd_grid"], st["bwd_grid"]) == (1026, 1024, 1024) and 32805 % 32 == 5
    assert by_name["widest"]["fwd_lds_bytes"] == 145408 <= 160 * 1024
    assert all(s["fwd_lds_bytes"] <= 160 * 1024 and s["bwd_lds_bytes"] <= 160 * 1024 for s in shapes.values())
    assert by_name["skip-last"]["head_segments"] == 2 and by_name["widest"]["head_segments"] == 2 and by_name["default"]["head_segments"] == 1
    rem = {c[1] % 32 for c in VR.CASES}
    assert {0, 1, 31} <= rem and any(1 < r < 31 for r in rem) and any(c[1] == 1 for c in VR.CASES)
    # both kinds of weight-gradient launch: one sample range per job (repeatable to the byte) and several (atomics in arrival order)
    assert {s["wgrad_split"] == 1 for s in shapes.values()} == {True, False}
    assert all(s["wgrad_split"] == 1 for c, s in shapes.items() if c[1] <= 511)
    # where the skip fires (after hidden layer i, mlp.py:92-96)
    fires = {k: [i for i in range(cfg["net_depth"]) if VR.skip_fires(cfg, i)] for k, (cfg, _, _) in VR.SHAPES.items()}
    assert fires == {"default": [4], "skip-last": [2], "widest": [1, 2], "narrow-net": [], "odd-tiles": [], "deepest": [5, 10], "second-trip": []}
    assert sum(VR.SHAPES["deepest"][0][k] for k in ("net_depth", "net_depth_condition")) + 2 == 16
