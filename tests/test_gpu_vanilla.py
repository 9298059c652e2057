"""GPU tests of the frequency-encoding + biased-MLP field (csrc/vanilla.hip, apnrf_amd/mlp.py) against the float64 restatement
tests/vanilla_ref.py, which tests/test_vanilla_ref_cpu.py holds to the definition.  The case table (vanilla_ref.SHAPES / CASES) reaches what
tests/test_gpu_parity.py's two tests of this unit do not: the constructor's default 8 x 256 shape, the width limits 32 and 512 and the 16-layer
limit, 1 to 4 waves per block in the forward and in the backward-data kernel, a second grid-stride trip, a skip that fires on the last hidden
layer (two-segment head), twice, or never, a condition net wider than the base net, and n = 1, 31, 32, 33.

Each case goes through the C ABI with canaries around every output and input, a training workspace of exactly
`mnf_vanilla_train_workspace_bytes` bytes prefilled with 0xFF (NaN) between canaries, twice, and compares the training forward, the inference
forward and `mnf_vanilla_density` to the byte.  The float canary is positive on purpose: a backward that read `sigma` / `d_sigma` of the tail
tile's missing samples would take the canary for a live sample.

Bars.  The project's bars for this unit (values atol 2e-6 + rtol 1e-5; gradients per tensor atol 2e-5 max|want| + 1e-9, rtol 1e-4), or 4 x the
fp32 noise floor of the operation where that is larger: the floor is the error of `evaluate(float32)` against `evaluate(float64)` on the CPU
(max abs for values; max abs / max|want| per gradient tensor), measured on the reference and never on the kernel.  The factor 4 covers the
MFMA's other summation order and the atomic accumulation across sample ranges.

Measured on one MI355X (achieved error / fp32 floor; gradients: the largest over the parameter tensors, relative to each tensor's max):

  case                     rgb                 sigma               gradients
  default-n1013            1.0e-07 / 9.4e-08   2.1e-07 / 1.5e-07   7.1e-07 / 1.2e-06
  default-n33              6.6e-08 / 6.8e-08   1.7e-07 / 7.6e-08   8.1e-07 / 5.8e-07
  skip-last-n333           1.2e-07 / 1.2e-07   3.7e-07 / 2.8e-07   8.0e-07 / 6.2e-07
  skip-last-n31            8.5e-08 / 8.0e-08   2.5e-07 / 2.8e-07   4.7e-07 / 3.9e-07
  widest-n333              2.2e-07 / 1.0e-07   3.9e-07 / 2.6e-07   1.1e-06 / 4.6e-07
  narrow-net-n64           8.7e-08 / 5.9e-08   2.1e-07 / 3.2e-07   7.9e-07 / 5.3e-07
  narrow-net-n1            3.8e-08 / 3.9e-08   4.8e-08 / 1.2e-08   1.9e-07 / 2.2e-07
  odd-tiles-n1013          1.2e-07 / 9.8e-08   5.6e-07 / 3.8e-07   3.5e-07 / 4.6e-07
  odd-tiles-n32            7.7e-08 / 7.2e-08   3.5e-07 / 2.9e-07   3.2e-07 / 3.9e-07
  deepest-n333             9.0e-08 / 9.0e-08   5.1e-07 / 4.1e-07   7.0e-07 / 5.2e-07
  second-trip-n32805       2.1e-07 / 1.9e-07   4.9e-07 / 3.5e-07   2.0e-06 / 6.4e-06
  odd-tiles-n333-r20       2.0e-07 / 2.3e-07   1.9e-06 / 1.4e-06   6.5e-07 / 2.8e-06
  default-broadcast        1.0e-07 / 9.2e-08   2.3e-07 / 1.4e-07   6.5e-07 / 5.2e-07
  odd-tiles-broadcast      9.5e-08 / 9.5e-08   3.3e-07 / 3.6e-07   4.6e-07 / 3.8e-07
  after Adam.step          2.3e-07 / 2.2e-07   1.6e-06 / 6.0e-07   -
  after load_state_dict    1.1e-07 / 1.1e-07   2.8e-07 / 2.6e-07   -
  after cpu -> device      1.4e-07 / 1.1e-07   4.2e-07 / 2.7e-07   -

The kernels sit at the floor of a CPU float32 evaluation everywhere, so the project's bars decide every case, second-trip's 32 805-sample sums
included: its floor is small here because vanilla_ref.make_case keeps every ReLU pre-activation clear of zero, so no sample changes the side of a
ReLU between float32 and float64 (one such flip moves a gradient by a whole sample's term, far above any relative bar).  Every case prints
its figures before it asserts (`pytest -s`).

With a scratch build of csrc/vanilla.hip that ignores the head's second input segment, the skip-last and widest cases and the parameter-update
test fail; without the `valid` guard on the raw-sigma row of the head's dZ pad rows, eleven of the sixteen tests here fail (the positive canary
after `sigma` and `d_sigma`).  Striding the forward's tile loop by gridDim.x instead of gridDim.x * waves changes no stored value: every tile is
still evaluated, some twice with the same result, so only a timing could see it.
"""
import functools

import numpy as np
import pytest
import torch

import vanilla_ref as VR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CANARY = 64                    # floats: 256 bytes, so what sits between two canaries keeps torch's allocation alignment (>= 16 bytes)
MARK = 12345.5
VAL_ATOL, VAL_RTOL, GRAD_ATOL, GRAD_RTOL, FLOOR_FACTOR = 2e-6, 1e-5, 2e-5, 1e-4, 4.0


def _lib():
    from apnrf_amd import _lib as L
    return L, L.load_library()


def _guarded(n, fill=None):
    whole = torch.full((n + 2 * CANARY,), MARK, dtype=torch.float32, device=DEV)
    part = whole[CANARY:CANARY + n]
    if fill is not None:
        part.copy_(fill.reshape(-1))
    return whole, part


def _assert_guards(whole, n, what):
    host = whole.cpu().numpy()
    assert (host[:CANARY] == MARK).all() and (host[CANARY + n:] == MARK).all(), f"{what}: written outside its bounds"


@functools.lru_cache(maxsize=None)
def _reference(case):
    """Computed once per case and shared: inputs, the float64 reference and the fp32 noise floors."""
    name, n, pos_range = case
    cfg, _, seed = VR.SHAPES[name]
    c = VR.make_case(cfg, n, seed, pos_range)
    return c, _ref_and_floor(c["sd"], cfg, c["x"], c["d"], c["g_rgb"], c["g_sigma"])


def _ref_and_floor(sd, cfg, x, d, g_rgb, g_sigma):
    rgb, sigma, grads = VR.evaluate(sd, cfg, x, d, g_rgb, g_sigma)
    rgb32, sigma32, grads32 = VR.evaluate(sd, cfg, x, d, g_rgb, g_sigma, dtype=torch.float32)
    floor = {"rgb": (rgb32.double() - rgb).abs().max().item() if rgb.numel() else 0.0,
             "sigma": (sigma32.double() - sigma).abs().max().item() if sigma.numel() else 0.0}
    for k, g in grads.items():
        floor[k] = ((grads32[k].double() - g).abs().max() / g.abs().max().clamp_min(1e-300)).item()
    return dict(rgb=rgb.numpy(), sigma=sigma.numpy(), grads={k: g.numpy() for k, g in grads.items()}, floor=floor)


def _check_values(tag, what, got, want, floor):
    got, want = np.asarray(got, np.float64).reshape(want.shape), np.asarray(want, np.float64)
    assert np.isfinite(got).all(), f"{tag} {what}: non-finite"
    err = np.abs(got - want)
    allowed = np.maximum(VAL_ATOL + VAL_RTOL * np.abs(want), FLOOR_FACTOR * floor)
    print(f"{tag} {what}: max err {err.max() if err.size else 0.0:.3e}, fp32 floor {floor:.3e}")
    assert (err <= allowed).all(), f"{tag} {what}: max err {err.max():.3e} (fp32 floor {floor:.3e}), worst excess {(err - allowed).max():.3e}"


def _check_grad(tag, name, got, want, floor):
    got, want = np.asarray(got, np.float64).reshape(want.shape), np.asarray(want, np.float64)
    assert np.isfinite(got).all(), f"{tag} grad {name}: non-finite"
    scale = np.abs(want).max()
    err = np.abs(got - want)
    allowed = np.maximum(GRAD_ATOL * scale + 1e-9 + GRAD_RTOL * np.abs(want), FLOOR_FACTOR * floor * scale)
    assert (err <= allowed).all(), f"{tag} grad {name}: max err / max|want| {err.max() / scale:.3e} (fp32 floor {floor:.3e})"
    return err.max() / scale


def _check_grads(tag, grads, ref):
    """`grads`: name -> array.  One line per call: the largest error and the largest floor over the parameter tensors."""
    rel = {k: _check_grad(tag, k, g, ref["grads"][k], ref["floor"][k]) for k, g in grads.items()}
    worst = max(rel, key=rel.get)
    print(f"{tag} gradients: largest max err / max|want| {rel[worst]:.3e} ({worst}), largest fp32 floor {max(ref['floor'][k] for k in rel):.3e}")


def _field(cfg, sd):
    from apnrf_amd.mlp import VanillaNeRFRadianceField
    field = VanillaNeRFRadianceField(**cfg)
    res = field.load_state_dict(sd, strict=False)
    assert set(res.missing_keys) == {"posi_encoder.scales", "view_encoder.scales"} and not res.unexpected_keys
    return field.to(DEV)


@pytest.mark.parametrize("case", VR.CASES, ids=VR.case_id)
def test_vanilla_c_abi_case(case):
    name, n, pos_range = case
    cfg = VR.SHAPES[name][0]
    c, ref = _reference(case)
    shape = VR.launch_shape(cfg, n)
    tag = VR.case_id(case)
    L, lib = _lib()
    field = _field(cfg, c["sd"])
    h, layout = field._ensure_handle(), field._layout
    names = [k for k, _ in field.named_parameters()]
    n_params = int(lib.mnf_vanilla_param_count(h))
    nbytes = int(lib.mnf_vanilla_train_workspace_bytes(h, n))
    assert nbytes == shape["workspace_bytes"], "vanilla_ref.launch_shape no longer restates csrc/vanilla.hip"
    assert len(layout) == len(names) and n_params == sum(r * k for _, r, k in layout)
    # inputs sit between canaries too: a read past their end meets a live-looking value, not whatever the allocator left there
    (_, x), (_, d) = _guarded(3 * n, c["x"].to(DEV)), _guarded(3 * n, c["d"].to(DEV))
    (_, g_rgb), (_, g_sigma) = _guarded(3 * n, c["g_rgb"].to(DEV)), _guarded(n, c["g_sigma"].to(DEV))
    pad = 4 * CANARY
    runs = []
    for _ in range(2):
        outs = {k: _guarded(m) for k, m in (("rgb", 3 * n), ("sigma", n), ("grad", n_params), ("rgb_inf", 3 * n), ("sigma_inf", n), ("sigma_den", n))}
        ws_whole = torch.full((nbytes + 2 * pad,), 0xA5, dtype=torch.uint8, device=DEV)
        ws = ws_whole[pad:pad + nbytes]
        ws.fill_(0xFF)                                                      # every float of the workspace is a NaN
        assert ws.data_ptr() % 16 == 0
        rgb, sigma, grad = outs["rgb"][1], outs["sigma"][1], outs["grad"][1]
        L.launch(lib.mnf_vanilla_forward, h, L.ptr(x), L.ptr(d), n, 1, L.ptr(rgb), L.ptr(sigma), L.ptr(ws), nbytes)
        L.launch(lib.mnf_vanilla_backward, h, L.ptr(g_rgb), L.ptr(g_sigma), L.ptr(rgb), L.ptr(sigma), n, L.ptr(ws), nbytes, L.ptr(grad))
        L.launch(lib.mnf_vanilla_forward, h, L.ptr(x), L.ptr(d), n, 1, L.ptr(outs["rgb_inf"][1]), L.ptr(outs["sigma_inf"][1]), None, 0)
        L.launch(lib.mnf_vanilla_density, h, L.ptr(x), n, L.ptr(outs["sigma_den"][1]))
        torch.cuda.synchronize()
        for k, (whole, part) in outs.items():
            _assert_guards(whole, part.numel(), k)
        assert (ws_whole[:pad] == 0xA5).all().item() and (ws_whole[pad + nbytes:] == 0xA5).all().item(), "workspace: written outside its bounds"
        runs.append({k: part.cpu().numpy() for k, (_, part) in outs.items()})
    a, b = runs
    for k in ("rgb", "sigma", "grad"):
        assert np.isfinite(a[k]).all(), f"{tag} {k}: non-finite out of a NaN-filled workspace"
    # inference paths
    assert a["sigma"].tobytes() == a["sigma_inf"].tobytes() == a["sigma_den"].tobytes()
    assert a["rgb"].tobytes() == a["rgb_inf"].tobytes()
    # repeatability
    for k in ("rgb", "sigma", "rgb_inf", "sigma_inf", "sigma_den"):
        assert a[k].tobytes() == b[k].tobytes(), k
    if shape["wgrad_split"] == 1:          # one sample range per job: every gradient element receives one atomic add onto zero
        assert a["grad"].tobytes() == b["grad"].tobytes()
    # values
    _check_values(tag, "rgb", a["rgb"], ref["rgb"], ref["floor"]["rgb"])
    _check_values(tag, "sigma", a["sigma"], ref["sigma"], ref["floor"]["sigma"])
    for run in runs:
        _check_grads(tag, {key: run["grad"][off:off + rows * cols] for key, (off, rows, cols) in zip(names, layout)}, ref)


@pytest.mark.parametrize("name", ["default", "odd-tiles"])
def test_direction_broadcast_across_tiles(name):
    """x [37, 7, 3] with condition [37, 3]: 7 samples per direction, so rays straddle the 32-sample tiles (`s / samples_per_direction`)."""
    cfg, _, seed = VR.SHAPES[name]
    rays, per_ray = 37, 7
    c = VR.make_case(cfg, rays * per_ray, seed + 100)
    x = c["x"].view(rays, per_ray, 3)
    d_ray = c["d"][::per_ray].contiguous()                                     # one direction per ray
    d_full = d_ray[:, None, :].expand(rays, per_ray, 3).contiguous()
    ref = _ref_and_floor(c["sd"], cfg, c["x"], d_full.reshape(-1, 3), c["g_rgb"], c["g_sigma"])
    field = _field(cfg, c["sd"])
    got = []
    for cond in (d_ray, d_full):
        field.zero_grad(set_to_none=True)
        rgb, sigma = field(x.to(DEV), cond.to(DEV))
        assert rgb.shape == (rays, per_ray, 3) and sigma.shape == (rays, per_ray, 1)
        torch.autograd.backward([rgb, sigma], [c["g_rgb"].view(rays, per_ray, 3).to(DEV), c["g_sigma"].view(rays, per_ray, 1).to(DEV)])
        with torch.no_grad():
            rgb_i, sigma_i = field(x.to(DEV), cond.to(DEV))
        assert torch.equal(rgb_i, rgb) and torch.equal(sigma_i, sigma)
        got.append((rgb.detach().cpu().numpy(), sigma.detach().cpu().numpy(), {k: p.grad.cpu().numpy() for k, p in field.named_parameters()}))
    (rgb, sigma, grads), (rgb_f, sigma_f, grads_f) = got
    assert rgb.tobytes() == rgb_f.tobytes() and sigma.tobytes() == sigma_f.tobytes()
    assert VR.launch_shape(cfg, rays * per_ray)["wgrad_split"] == 1
    assert all(grads[k].tobytes() == grads_f[k].tobytes() for k in grads)
    tag = f"{name}-broadcast"
    _check_values(tag, "rgb", rgb, ref["rgb"], ref["floor"]["rgb"])
    _check_values(tag, "sigma", sigma, ref["sigma"], ref["floor"]["sigma"])
    _check_grads(tag, grads, ref)


def test_empty_batch_under_autograd():
    cfg, _, seed = VR.SHAPES["odd-tiles"]
    c = VR.make_case(cfg, 32, seed)
    field = _field(cfg, c["sd"])
    rgb, sigma = field(torch.zeros(0, 3, device=DEV), torch.zeros(0, 3, device=DEV))
    assert rgb.shape == (0, 3) and sigma.shape == (0, 1) and rgb.requires_grad and sigma.requires_grad
    (rgb.sum() + sigma.sum()).backward()
    torch.cuda.synchronize()
    for k, p in field.named_parameters():
        assert p.grad is not None and p.grad.shape == p.shape and (p.grad == 0).all().item(), k
    assert field.query_density(torch.zeros(0, 3, device=DEV)).shape == (0, 1)


def test_parameter_updates_are_seen():
    """The library holds its own copy of the parameters (flat, and as MFMA fragments): after an optimizer step, a `load_state_dict` and a
    trip through the CPU the next forward must follow the module's CURRENT parameters."""
    name = "skip-last"
    cfg, _, seed = VR.SHAPES[name]
    c, _ = _reference((name, 333, 1.5))
    x, d, zeros = c["x"], c["d"], torch.zeros(333, 3)
    field = _field(cfg, c["sd"])

    def check(tag, previous):
        sd = {k: v.detach().cpu() for k, v in field.state_dict().items()}
        ref = _ref_and_floor(sd, cfg, x, d, zeros, zeros[:, 0])
        with torch.no_grad():
            rgb, sigma = field(x.to(DEV), d.to(DEV))
        rgb, sigma = rgb.cpu().numpy(), sigma.cpu().numpy()[:, 0]
        _check_values(tag, "rgb", rgb, ref["rgb"], ref["floor"]["rgb"])
        _check_values(tag, "sigma", sigma, ref["sigma"], ref["floor"]["sigma"])
        assert np.array_equal(field.query_density(x.to(DEV)).cpu().numpy()[:, 0], sigma)
        if previous is not None:      # the step really moved the outputs: following stale parameters could not pass the check above
            assert np.abs(rgb - previous).max() > 1e-3
        return rgb

    out = check("initial", None)
    opt = torch.optim.Adam(field.parameters(), lr=1e-2)
    rgb, sigma = field(x.to(DEV), d.to(DEV))
    torch.autograd.backward([rgb, sigma], [c["g_rgb"].to(DEV), c["g_sigma"].view(-1, 1).to(DEV)])
    opt.step()
    out = check("after Adam.step", out)
    other = VR.make_case(cfg, 32, seed + 1)["sd"]
    field.load_state_dict(other, strict=False)
    out = check("after load_state_dict", out)
    field = field.cpu()
    field.load_state_dict(VR.make_case(cfg, 32, seed + 2)["sd"], strict=False)
    field = field.to(DEV)
    out = check("after cpu -> device", out)
    field = field.cpu().to(DEV)                                              # the plain round trip: same values, new storage
    again = check("after plain round trip", None)
    assert again.tobytes() == out.tobytes()
