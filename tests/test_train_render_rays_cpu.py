"""`render.fused_train_render_rays` without a GPU: it is `fused_train_render` under another name as far as a caller's arguments go."""
import inspect

from apnrf_amd import render as RD


def test_signature_is_fused_train_renders():
    mine, ref = inspect.signature(RD.fused_train_render_rays).parameters, inspect.signature(RD.fused_train_render).parameters
    assert list(mine) == list(ref)
    assert all(mine[k].default == ref[k].default and mine[k].kind == ref[k].kind for k in ref)
