"""Float64 restatement of the frequency-encoding + biased-MLP field (the reference's perception/models/radiance_fields/mlp.py:14-245:
`MLP`, `NerfMLP`, `SinusoidalEncoder`, `VanillaNeRFRadianceField`) in plain torch on the CPU with autograd, the case table of
tests/test_gpu_vanilla.py, and a restatement of the host arithmetic of csrc/vanilla.hip that decides which launch route a case takes.
Written from the reference's definition, not from the product's Python; tests/test_vanilla_ref_cpu.py holds it to the golden-anchored
oracle (oracle/vanilla.py) and to a torch.nn evaluation of the same parameter tree.

Parameters are addressed by the product's (= the reference's) `state_dict` names."""
import math

import torch

POS_DEG, DIR_DEG = 10, 4
HALF_PI_F32 = torch.tensor(0.5 * math.pi, dtype=torch.float32)

# name -> (constructor arguments, sample counts, seed).  The waves named in the comments are asserted through `launch_shape` by
# tests/test_vanilla_ref_cpu.py::test_route_coverage.
SHAPES = {
    "default":     (dict(net_depth=8, net_width=256, skip_layer=4, net_depth_condition=1, net_width_condition=128), (1013, 33), 11),     # 1 / 2 waves
    "skip-last":   (dict(net_depth=3, net_width=160, skip_layer=2, net_depth_condition=2, net_width_condition=192), (333, 31), 12),      # 2 / 3
    "widest":      (dict(net_depth=3, net_width=512, skip_layer=1, net_depth_condition=1, net_width_condition=512), (333,), 13),         # 1 / 1
    "narrow-net":  (dict(net_depth=2, net_width=32, skip_layer=None, net_depth_condition=1, net_width_condition=512), (64, 1), 14),      # 1 / 1
    "odd-tiles":   (dict(net_depth=2, net_width=96, skip_layer=7, net_depth_condition=3, net_width_condition=32), (1013, 32), 15),       # 3 / 4
    "deepest":     (dict(net_depth=12, net_width=32, skip_layer=5, net_depth_condition=2, net_width_condition=32), (333,), 16),          # 4 / 4
    "second-trip": (dict(net_depth=1, net_width=320, skip_layer=None, net_depth_condition=1, net_width_condition=32), (32805,), 17),     # 1 / 1
}
# (shape name, n, pos_range): positions uniform in +-1.5, and one odd-tiles case at the extent of the project's scenes (sine arguments ~1e4)
CASES = [(name, n, 1.5) for name, (_, ns, _) in SHAPES.items() for n in ns] + [("odd-tiles", 333, 20.0)]


def case_id(case):
    name, n, pos_range = case
    return f"{name}-n{n}" + ("" if pos_range == 1.5 else f"-r{pos_range:g}")


def skip_fires(cfg, i):
    """mlp.py:50-54 / :92-96: the concat happens AFTER hidden layer i."""
    s = cfg["skip_layer"]
    return s is not None and i % s == 0 and i > 0


def param_shapes(cfg):
    """name -> shape, in the reference's `named_parameters()` order (base, sigma layer, bottleneck layer, rgb layer)."""
    e_dim, c_dim = 3 + 6 * POS_DEG, 3 + 6 * DIR_DEG
    W, Wc = cfg["net_width"], cfg["net_width_condition"]
    out, width_in = {}, e_dim

    def lin(name, o, i):
        out[name + ".weight"], out[name + ".bias"] = (o, i), (o,)

    for i in range(cfg["net_depth"]):
        lin(f"mlp.base.hidden_layers.{i}", W, width_in)
        width_in = W + e_dim if skip_fires(cfg, i) else W
    lin("mlp.sigma_layer.output_layer", 1, width_in)
    lin("mlp.bottleneck_layer.output_layer", W, width_in)
    width_in = W + c_dim
    for i in range(cfg["net_depth_condition"]):
        lin(f"mlp.rgb_layer.hidden_layers.{i}", Wc, width_in)
        width_in = Wc
    lin("mlp.rgb_layer.output_layer", 3, width_in)
    return out


def encode(v, deg, dtype=torch.float64):
    """mlp.py:187-203.  The sine's ARGUMENT is formed in float32 as the definition does (`x * 2^i` is exact, `+ float32(0.5 pi)` is one float32
    rounding) and only then widened, so that nothing but the sine's own error separates a float32 evaluation from this one."""
    v = v.to(torch.float32)
    scales = torch.tensor([2.0 ** i for i in range(deg)], dtype=torch.float32)
    xb = (v[..., None, :] * scales[:, None]).reshape(*v.shape[:-1], deg * v.shape[-1])
    arg = torch.cat([xb, xb + HALF_PI_F32], -1)
    assert arg.dtype == torch.float32
    return torch.cat([v.to(dtype), torch.sin(arg.to(dtype))], -1)


def forward(params, cfg, x, d, dtype=torch.float64):
    """-> rgb [n,3], sigma [n], raw sigma [n], the pre-activations of every hidden layer (base, then rgb layer)."""
    def lin(h, name):
        return h @ params[name + ".weight"].t() + params[name + ".bias"]

    e = encode(x, POS_DEG, dtype)
    h, pre = e, []
    for i in range(cfg["net_depth"]):
        pre.append(lin(h, f"mlp.base.hidden_layers.{i}"))
        h = torch.relu(pre[-1])
        if skip_fires(cfg, i):
            h = torch.cat([h, e], -1)
    raw_sigma = lin(h, "mlp.sigma_layer.output_layer")[:, 0]
    z = torch.cat([lin(h, "mlp.bottleneck_layer.output_layer"), encode(d, DIR_DEG, dtype)], -1)
    for i in range(cfg["net_depth_condition"]):
        pre.append(lin(z, f"mlp.rgb_layer.hidden_layers.{i}"))
        z = torch.relu(pre[-1])
    rgb = torch.sigmoid(lin(z, "mlp.rgb_layer.output_layer"))
    return rgb, torch.relu(raw_sigma), raw_sigma, pre


def evaluate(state_dict, cfg, x, d, g_rgb, g_sigma, dtype=torch.float64):
    """-> rgb [n,3], sigma [n], {name: gradient of sum(rgb * g_rgb) + sum(sigma * g_sigma)}, all in `dtype`.  float64 is the reference;
    float32 is the plain fp32 evaluation whose error against float64 is the noise floor of the operation itself."""
    params = {k: torch.as_tensor(v).detach().to(dtype).clone().requires_grad_(True) for k, v in state_dict.items() if k.startswith("mlp.")}
    rgb, sigma, _, _ = forward(params, cfg, x, d, dtype)
    torch.autograd.backward([rgb, sigma], [g_rgb.to(dtype).reshape(-1, 3), g_sigma.to(dtype).reshape(-1)])
    return rgb.detach(), sigma.detach(), {k: p.grad for k, p in params.items()}


RELU_MARGIN = 1e-5
CALIBRATION = 1024


def make_case(cfg, n, seed, pos_range=1.5):
    """-> dict(sd, x [n,3], d [n,3], g_rgb [n,3], g_sigma [n]), float32.

    Xavier-uniform weights, biases uniform in +-0.1, positions uniform in +-pos_range, unit directions, normal upstream gradients.  The sigma
    layer's bias is shifted by minus the median of the float64 raw sigma so that the sigma ReLU is on for about half the samples (with the plain
    initialisation the default 8 x 256 shape has sigma > 0 on every sample, and its relu' mask would go untested).  The median is taken over
    CALIBRATION positions of the same distribution drawn before the case's own, not over the case's samples: the parameters then do not depend
    on n (the sample counts of one shape share them), and no sample is parked at raw sigma = 0, where rounding would pick the ReLU's side.

    For the same reason the case's samples are the first n of a longer draw whose every ReLU pre-activation, hidden layers and raw sigma, is at
    least RELU_MARGIN away from zero in float64 (fp32 errors of these pre-activations are ~1e-6): on such inputs a float32 evaluation takes
    the same side of every ReLU as the reference, which is what makes its gradients comparable with a relative bar at all."""
    g = torch.Generator().manual_seed(seed)

    def uniform(shape, bound):
        return (torch.rand(shape, generator=g, dtype=torch.float64) * 2 - 1).mul(bound).to(torch.float32)

    sd = {}
    for name, shape in param_shapes(cfg).items():
        sd[name] = uniform(shape, math.sqrt(6.0 / (shape[0] + shape[1])) if len(shape) == 2 else 0.1)
    p64 = {k: v.double() for k, v in sd.items()}
    calib = uniform((CALIBRATION, 3), pos_range)
    raw = forward(p64, cfg, calib, torch.zeros(CALIBRATION, 3))[2]
    sd["mlp.sigma_layer.output_layer.bias"] = (sd["mlp.sigma_layer.output_layer.bias"].double() - raw.median()).to(torch.float32)
    p64 = {k: v.double() for k, v in sd.items()}
    m = n + max(64, n // 2)
    x = uniform((m, 3), pos_range)
    d = torch.nn.functional.normalize(torch.randn(m, 3, generator=g, dtype=torch.float64), dim=-1).to(torch.float32)
    g_rgb, g_sigma = torch.randn(m, 3, generator=g), torch.randn(m, generator=g)
    _, _, raw, pre = forward(p64, cfg, x, d)
    clear = raw.abs() > RELU_MARGIN
    for z in pre:
        clear &= z.abs().min(dim=-1).values > RELU_MARGIN
    keep = torch.nonzero(clear)[:n, 0]
    assert keep.numel() == n, f"only {keep.numel()} of {m} samples clear every ReLU by {RELU_MARGIN}"
    return dict(sd=sd, x=x[keep].contiguous(), d=d[keep].contiguous(), g_rgb=g_rgb[keep].contiguous(), g_sigma=g_sigma[keep].contiguous())


def launch_shape(cfg, n):
    """The host arithmetic of csrc/vanilla.hip that picks a case's launch route, restated.  THIS FUNCTION MUST BE UPDATED TOGETHER WITH
    `pick_waves` AND THE LAUNCH CODE IT MIRRORS: the tests cannot ask the library which route a case took, so this is how they know that every
    route is covered.  tests/test_gpu_vanilla.py compares `workspace_bytes` with the library's own answer, which catches a drift of the
    layer chain; the waves have no such check.

    Mirrors, in csrc/vanilla.hip:
      build_net            the layer chain (hidden layers, head = bottleneck + raw sigma, rgb hidden layers, rgb output), `buf_rows` = the largest
                           padded output that is staged in LDS = max(net_width + 8, net_width_condition), `act_rows`, and the weight-gradient
                           jobs: one per (layer, 32-row output tile, 32-row tile of the padded input)
      fwd_lds_bytes        (64 + 32 + 2 * buf_rows) * 32 * 4 bytes per wave
      bwd_lds_bytes        2 * buf_rows * 32 * 4 bytes per wave
      pick_waves           floor(150 KiB / bytes per wave), at most 4
      vanilla_forward, mnf_vanilla_backward
                           tiles = ceil(n / 32), grid = min(1024, ceil(tiles / waves)); the weight-gradient split = 2048 / jobs, at most tiles / 8,
                           at least 1
      mnf_vanilla_train_workspace_bytes
                           max(tiles, 1) * act_rows * 32 * 4
    """
    D, W, Dc, Wc = cfg["net_depth"], cfg["net_width"], cfg["net_depth_condition"], cfg["net_width_condition"]
    layers, prev_pad, concat = [], 64, False          # (n_out, padded input rows)
    for i in range(D):
        layers.append((W, prev_pad + (64 if concat else 0)))
        prev_pad, concat = W, skip_fires(cfg, i)
    head_segments = 2 if concat else 1
    layers.append((W + 1, prev_pad + (64 if concat else 0)))
    for i in range(Dc):
        layers.append((Wc, W + 32 if i == 0 else Wc))
    layers.append((3, Wc))
    pad8 = lambda v: (v + 7) // 8 * 8
    buf_rows = max([8] + [pad8(o) for o, _ in layers[:-1]])
    assert buf_rows == max(W + 8, Wc)
    act_rows = 64 + 32 + D * W + W + Dc * Wc + sum(pad8(o) for o, _ in layers)
    jobs = sum(((o + 31) // 32) * ((i + 31) // 32) for o, i in layers)
    fwd_bytes, bwd_bytes = (64 + 32 + 2 * buf_rows) * 128, 2 * buf_rows * 128
    tiles = (n + 31) // 32
    out = dict(buf_rows=buf_rows, act_rows=act_rows, tiles=tiles, head_segments=head_segments, jobs=jobs,
               workspace_bytes=max(tiles, 1) * act_rows * 128)
    for key, per_wave in (("fwd", fwd_bytes), ("bwd", bwd_bytes)):
        waves = min(4, 150 * 1024 // per_wave)
        grid = min(1024, -(-tiles // waves)) if tiles else 0
        out[key + "_waves"], out[key + "_lds_bytes"], out[key + "_grid"] = waves, waves * per_wave, grid
        out[key + "_second_trip"] = tiles > grid * waves
    out["wgrad_split"] = max(1, min(2048 // jobs, tiles // 8))
    return out
