"""Child process of test_dead_tiles_skip_heads_and_compositing_without_moving_a_bit: runs under MNF_LIB_PATH=libmi355nerf_diag.so (the -DMNF_DIAG build, the only
one that reads MNF_NO_TILE_SKIP / MNF_MIN_SAMPLES / MNF_ROUND_LOG).  A render tile (64 columns) in which no sample passes the alpha threshold stops behind the density
(csrc/field.hip): no heads, no compositing, only its rays' retirement.  Every output must keep its bits against the same render with the skip switched off, for every
slot form (strides 4 / 8 / 16 on the diagnostic schedules, the reference schedule's other strides down the general path) and in probabilistic mode; and the round log
must show a round with dead AND live tiles, so that both branches really ran."""
import os
import re
import sys
import tempfile

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import helpers as H  # noqa: E402
from apnrf_amd import _lib as L  # noqa: E402
from apnrf_amd import render as RD  # noqa: E402
from test_gpu_tile_skip import DENSITY_ROW_SCALE, scale_density_row  # noqa: E402

assert L.lib_path().endswith("_diag.so"), L.lib_path()
DEV = "cuda:0"
LOG = re.compile(r"\[mnf round (\d+)\].* budgets (\d+).* tiles (\d+) dead (\d+)  live_rays (\d+) idle (\d+)")      # (one view per call here: one budget)


def logged(fn):
    """fn() with the library's stderr (the MNF_ROUND_LOG lines) caught: [(round, budget, tiles, dead, live_rays, idle)]"""
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile(mode="w+b") as tmp:
        os.dup2(tmp.fileno(), 2)
        try:
            out = fn()
            torch.cuda.synchronize()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        text = tmp.read().decode(errors="replace")
    return out, [tuple(int(x) for x in m.groups()) for m in map(LOG.search, text.splitlines()) if m]


scene = scale_density_row(H.make_scene(), DENSITY_ROW_SCALE)      # (why: test_gpu_tile_skip.py)
hip, est = H.hip_field(scene), H.hip_estimator(scene)
oa, da = H.view_rays(scene, 2, h=48, w=48)
ob, db = H.view_rays(scene, 5, h=48, w=48)
o, d = torch.cat([oa, ob, oa[:150]]).to(DEV), torch.cat([da, db, da[:150]]).to(DEV)      # ragged: the last march workgroup is partly idle
os_, ds_ = H.view_rays(scene, 1, h=40, w=40)
bk = torch.zeros(3)
os.environ["MNF_ROUND_LOG"] = "1"
cases = [(str(ms), prob, o, d) for ms, prob in [(4, False), (4, True), (8, True), (16, False)]]
cases += [(None, False, os_.to(DEV), ds_.to(DEV)), (None, True, os_.to(DEV), ds_.to(DEV))]      # the reference's schedule on one small view: strides 1600 // n_alive
for min_samples, prob, ro, rd in cases:
    n = ro.shape[0]
    if min_samples is None:
        os.environ.pop("MNF_MIN_SAMPLES", None)
    else:
        os.environ["MNF_MIN_SAMPLES"] = min_samples

    def render():
        return RD.render_views(hip, est, ro, rd, n, 1024, render_bkgd=bk, probabilistic=prob, **H.RENDER_KW)

    os.environ.pop("MNF_NO_TILE_SKIP", None)
    skip, rounds = logged(render)
    os.environ["MNF_NO_TILE_SKIP"] = "1"
    full, rounds_full = logged(render)
    assert int(skip["total"][1]) > 20 * n, skip["total"]                                  # the schedule really ran
    for k in ("rgb", "acc", "depth", "sem", "total") + (("rgb_var", "depth_var") if prob else ()):
        assert torch.equal(skip[k], full[k]), (min_samples, prob, k, float((skip[k].double() - full[k].double()).abs().max()))
    mixed = [r for r in rounds if 0 < r[3] < r[2]]
    assert mixed, (min_samples, prob, rounds)                                            # a round with dead and live tiles: both branches ran
    assert all(r[3] == 0 for r in rounds_full) and [r[:3] for r in rounds_full] == [r[:3] for r in rounds]      # the switch really switches; same schedule, same tiles
    if min_samples is None:                                                              # the general path had dead and live tiles too
        assert [r for r in mixed if r[1] not in (4, 8, 16)], rounds
    print("case", min_samples, prob, "ok: rounds", len(rounds), "of them mixed", len(mixed), "strides", sorted({r[1] for r in mixed}), "tiles", sum(r[2] for r in rounds),
          "dead", sum(r[3] for r in rounds), "rays of live tiles", sum(r[4] for r in rounds), "of them without a kept sample", sum(r[5] for r in rounds), flush=True)
print("DIAG_TILE_SKIP_OK")
