"""`render.fused_train_render` without a GPU: its signature against the drop-in's, and — with the launcher stubbed — what it decides from the four counters
of a launch: repeat with larger bounds, hand over to `render_image_with_occgrid_with_depth_guide`, give up; `train_step` refuses `loss_fn` with sync=False."""
import inspect
import types

import pytest
import torch

from apnrf_amd import render as RD


class _Field:
    training = True
    num_semantic_classes = 5

    def parameters(self):
        return []


def _estimator(levels=1):
    return types.SimpleNamespace(levels=levels, last_sampling=None)


def _rays(n=7):
    return RD.Rays(torch.zeros(n, 3), torch.ones(n, 3))


def _stub_launcher(monkeypatch, reports):
    """`_launch_train_render` replaced by a script of (marched, kept, longest, status) reports; logs the bounds each attempt was launched with"""
    calls = []

    def launch(st, field, estimator, rays, render_bkgd, seed, own_workspace, **opts_kw):
        R = rays.origins.reshape(-1, 3).shape[0]
        calls.append(dict(caps=st.caps(R), seed=seed, own_workspace=own_workspace, opts=opts_kw))
        c = reports[len(calls) - 1]
        return dict(rgb=torch.full((R, 3), float(len(calls))), acc=torch.zeros(R, 1), depth=torch.zeros(R, 1), sem=torch.zeros(R, field.num_semantic_classes),
                    counts=torch.tensor(c, dtype=torch.int64), skip=torch.tensor(int(c[3] != 0), dtype=torch.int32), _rays=R)
    monkeypatch.setattr(RD, "_launch_train_render", launch)
    return calls


def _stub_drop_in(monkeypatch):
    calls = []

    def drop_in(field, estimator, rays, **kw):
        calls.append(dict(kw, training=field.training))
        return "rgb", "acc", "depth", "sem", 123
    monkeypatch.setattr(RD, "render_image_with_occgrid_with_depth_guide", drop_in)
    return calls


def test_signature_mirrors_the_drop_in():
    mine, ref = inspect.signature(RD.fused_train_render).parameters, inspect.signature(RD.render_image_with_occgrid_with_depth_guide).parameters
    shared = ["radiance_field", "estimator", "rays", "near_plane", "far_plane", "render_step_size", "render_bkgd", "cone_angle", "alpha_thre"]
    assert list(mine)[:9] == shared == list(ref)[:9]
    assert all(mine[k].default == ref[k].default for k in shared) and mine["depth"].default is None and "depth" in ref
    assert list(mine)[9:] == ["early_stop_eps", "depth", "stratified", "seed", "deterministic"]
    assert (mine["early_stop_eps"].default, mine["stratified"].default, mine["seed"].default, mine["deterministic"].default) == (1e-4, None, None, False)


def test_result_has_the_drop_ins_arity_and_shapes(monkeypatch):
    calls = _stub_launcher(monkeypatch, [(900, 400, 200, 0)])
    f, est = _Field(), _estimator()
    rays = RD.Rays(torch.zeros(2, 3, 3), torch.ones(2, 3, 3))
    out = RD.fused_train_render(f, est, rays, near_plane=0.1, alpha_thre=0.01, seed=5, depth=torch.zeros(6))
    assert len(out) == 5 and out[4] == 400 and isinstance(out[4], int)
    assert out[0].shape == (2, 3, 3) and out[1].shape == (2, 3, 1) and out[2].shape == (2, 3, 1) and out[3].shape == (2, 3, 5)
    assert len(calls) == 1 and calls[0]["seed"] == 5 and calls[0]["own_workspace"] is False      # no parameter wants a gradient: the cached slot will do
    assert calls[0]["opts"] == dict(near_plane=0.1, far_plane=1e10, render_step_size=1e-3, cone_angle=0.0, alpha_thre=0.01, early_stop_eps=1e-4, stratified=None,
                                    deterministic=False)
    assert est.last_sampling == {"n_marched": 900}
    last = RD.latest_train_render(f)
    assert last["counts"].tolist() == [900, 400, 200, 0] and int(last["skip"]) == 0


def test_overflow_grows_the_bounds_and_repeats(monkeypatch):
    big = 5_000_000
    calls = _stub_launcher(monkeypatch, [(big, 0, 300, RD._ST_MARCHED | RD._ST_EMPTY), (big, 4_000_000, 300, RD._ST_KEPT), (big, 4_000_000, 300, 0)])
    f = _Field()
    out = RD.fused_train_render(f, _estimator(), _rays(7), seed=1)
    want = RD.TrainState()
    caps = [want.caps(7)]
    want.grow(big, 0, 7, carry=False); caps.append(want.caps(7))
    want.grow(big, 4_000_000, 7, carry=False); caps.append(want.caps(7))
    assert [c["caps"] for c in calls] == caps and caps[0] < caps[1] < caps[2]
    assert len({c["seed"] for c in calls}) == 1                                            # one jitter seed, whatever the number of attempts
    assert out[4] == 4_000_000 and float(out[0][0, 0]) == 3.0                              # the third attempt's planes
    assert RD._train_state(f).caps(7) == caps[2] and RD._train_state(f).caps(8) == RD.TrainState().caps(8)      # carry=False: this ray count only


def test_bounds_that_keep_growing_raise(monkeypatch):
    calls = _stub_launcher(monkeypatch, [(10 ** (7 + k), 0, 300, RD._ST_MARCHED) for k in range(5)])
    with pytest.raises(RD.L.MnfError, match="kept growing"):
        RD.fused_train_render(_Field(), _estimator(), _rays(), seed=1)
    assert len(calls) == 4


def test_more_than_four_levels_and_a_row_overflow_hand_over(monkeypatch):
    launches = _stub_launcher(monkeypatch, [(5000, 0, 3000, RD._ST_ROW | RD._ST_EMPTY)])
    drop_in = _stub_drop_in(monkeypatch)
    f = _Field()
    kw = dict(near_plane=0.1, render_step_size=2e-3, cone_angle=0.004, alpha_thre=0.01, render_bkgd=None)
    assert RD.fused_train_render(f, _estimator(levels=5), _rays(), seed=1, **kw) == ("rgb", "acc", "depth", "sem", 123)
    assert launches == [] and len(drop_in) == 1 and RD.latest_train_render(f) is None
    assert drop_in[0] == dict(kw, far_plane=1e10, depth=None, training=True)
    # status bit 2 (a ray past the sampler's scratch row): one launch, then the drop-in; stratified=False is honoured by rendering in eval mode
    f.train, f.eval = (lambda: setattr(f, "training", True)), (lambda: setattr(f, "training", False))
    assert RD.fused_train_render(f, _estimator(), _rays(), seed=1, stratified=False, **kw)[4] == 123
    assert len(launches) == 1 and len(drop_in) == 2 and drop_in[1]["training"] is False and f.training is True
    assert RD.latest_train_render(f) is None


def test_train_step_refuses_a_loss_fn_without_sync():
    with pytest.raises(ValueError, match="loss_fn"):
        RD.train_step(_Field(), _estimator(), None, _rays(), None, None, None, None, step=1, sync=False, loss_fn=lambda *a: a[0].sum())
    assert "loss_fn" in inspect.signature(RD.train_step).parameters and inspect.signature(RD.train_step).parameters["loss_fn"].default is None
