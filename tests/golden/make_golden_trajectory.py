"""Generate tests/golden/trajectory.npz by RUNNING THE REFERENCE's `ActiveNeRFMapper.trajector_uncertainty`
(scripts/pipeline.py:800-916), the ensemble-disagreement trajectory scorer.

Run in the build container only (it needs the reference checkout, as make_golden.py does):

    python tests/golden/make_golden_trajectory.py

Scene, fields (the oracle's NGP field, parameter seeds 0 and 1, log2_hashmap_size 14), estimators, the 60-pose trajectory and
W = H = 50 are those of `gen_scorer` (make_golden.py), imported from it; the trajectory is read from scorer.npz, which that
generator wrote.  At the method's scale = 0.1 a view has 5 x 5 = 25 pixels.

ONE wrapper stands between the method and `Dataset.render_image_from_pose`.  With `num_semantic_classes > 0` and more than one
member the unmodified method cannot run: `render_image_from_pose` returns four arrays whenever the field has classes, and
pipeline.py:840 unpacks three (`ValueError: too many values to unpack (expected 3)`).  The wrapper records each call's outputs and
hands the method `out[:3]` for every member after the first.  It does nothing else; the method body runs unmodified.

The method is run for step = 1 and for step = -1 on a stand-in `self` whose `trajector_uncertainty_list` is `[[], []]`
(`step == -1` indexes `[-2]`, so the list needs two lists; both steps append to the first).

Stored: the scene keys of scorer.npz; `unc_idx`; both members' `images`, `depths`, `accs` and member 0's `sems` as fp32 (the
float64 stacks are widened fp32 renders: asserted); the four clipped rows `rows` [4,40] and `max_idx` (the same for
both steps: asserted) and the two returned uncertainties `unc_step1`, `unc_stepm1`.
"""
import os
import sys

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, OUT)                                     # make_golden.py, ref_shim.py
sys.path.insert(0, os.path.dirname(os.path.dirname(OUT)))   # the repository root: apnrf_amd, oracle


def gen_trajectory():
    from make_golden import GLUE_KW, _glue_scene, _ngp_fields, _ref_estimator
    import ref_shim
    ref_shim.enter_reference(with_pipeline=True)
    import pipeline as P
    import habitat_to_data as h2d
    scorer = np.load(os.path.join(OUT, "scorer.npz"))
    sc = _glue_scene()
    fields, sums = _ngp_fields(sc, [0, 1], 14)
    ests = [_ref_estimator(sc), _ref_estimator(sc)]
    W = H = 50
    focal = 0.5 * W / np.tan(np.pi / 4)
    traj = scorer["trajectory"]
    assert traj.shape == (60, 7) and np.array_equal(scorer["whf"], np.asarray([W, H, focal])) and np.array_equal(scorer["param_sums"], sums)

    class Self:
        config_file = dict(n_ensembles=2, cuda="cpu", img_w=W, img_h=H, sample_disc=35, **GLUE_KW)
        radiance_fields, estimators = fields, ests
    Self.focal = focal
    real = h2d.Dataset.render_image_from_pose
    stacks = []

    def recording(radiance_field, *a, **k):
        out = real(radiance_field, *a, **k)
        stacks.append(out)
        return out if radiance_field is fields[0] else out[:3]
    P.Dataset.render_image_from_pose = staticmethod(recording)
    runs = {}
    try:
        for tag, step in (("step1", 1), ("stepm1", -1)):
            me = Self()
            me.trajector_uncertainty_list = [[], []]
            del stacks[:]
            unc, max_idx = P.ActiveNeRFMapper.trajector_uncertainty(me, traj, step)
            assert len(me.trajector_uncertainty_list[0]) == 1 and not me.trajector_uncertainty_list[1] and len(stacks) == 2
            runs[tag] = (np.float64(unc), np.asarray(max_idx), np.asarray(me.trajector_uncertainty_list[0][0], np.float64), list(stacks))
    finally:
        P.Dataset.render_image_from_pose = staticmethod(real)
    a = np.linspace(0, len(traj) - 20, 20); b = np.linspace(len(traj) - 20, len(traj) - 1, 20)
    unc_idx = np.hstack((a, b)).astype(int)
    rec = dict(aabb=sc["aabb"], res=np.asarray(sc["res"]), occ=np.packbits(sc["occ"]), occs=sc["occs"], param_seeds=np.asarray([0, 1]),
               log2_hashmap_size=np.int64(14), param_sums=sums, trajectory=traj, unc_idx=unc_idx, whf=np.asarray([W, H, focal]),
               **{"kw_" + k: np.float64(v) for k, v in GLUE_KW.items()})
    for tag, (unc, max_idx, rows, _) in runs.items():
        assert rows.shape == (4, 40)
        assert np.array_equal(rows, runs["step1"][2]) and np.array_equal(max_idx, runs["step1"][1])     # neither depends on the step
        rec["unc_" + tag] = unc
    rec["rows"], rec["max_idx"] = runs["step1"][2], runs["step1"][1]
    s1, sm1 = runs["step1"][3], runs["stepm1"][3]
    for m in range(2):
        for nm, arr, again in zip(("images", "depths", "accs", "sems"), s1[m], sm1[m]):
            assert np.array_equal(arr, again)                                          # the renders do not depend on the step
            assert np.array_equal(arr.astype(np.float32).astype(np.float64), arr)      # fp32 renders widened: stored as fp32 without loss
            if nm != "sems" or m == 0:
                rec[f"m{m}_{nm}"] = arr.astype(np.float32)
    np.savez_compressed(os.path.join(OUT, "trajectory.npz"), **rec)


if __name__ == "__main__":
    gen_trajectory()
    print("wrote trajectory")
