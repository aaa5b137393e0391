"""The f15 specification on the oracle alone (no GPU): the named scenes of tests/computepose_ref.py reach every action and branch
of computePose, and every scene and ceresPnP case the GPU test uses meets the margin conditions, so that no decision of that
test hangs on the last bits of a sum."""
import numpy as np
import pytest

from tests import computepose_ref as R
from tests import p3p_ref


def test_named_scenes_reach_every_action_and_branch(oracle):
    got = {}
    for name, (sk, pk, action, pred) in R.SCENES.items():
        params, pb, ref = R.named_scene(oracle, name)
        assert ref["action"] == action, name
        got[name] = ref
        print(name, "action", ref["action"], "removed by p3p", ref["n_removed_p3p"], "pnp outliers", ref["n_outliers_pnp"],
              "passes", [q["ran"] for q in ref["passes"]], "p3p status", ref["p3p"]["status"])
    assert {r["action"] for r in got.values()} == {R.TOO_FEW, R.POSE_OK, R.PNP_REQ_P3P, R.P3P_RESET, R.PNP_RESET, R.PNP_KEEP}
    # TOO_FEW: nothing ran, nothing changed
    r = got["too_few"]
    assert not r["ran_p3p"] and not r["passes"][0]["ran"] and not r["removed"].any()
    # POSE_OK without P3P (two passes), with P3P (removals of both kinds), without outliers (no pass 2), with apply_l2 off
    r = got["ok_no_p3p"]
    assert not r["ran_p3p"] and r["passes"][0]["ran"] and r["passes"][1]["ran"] and set(np.unique(r["removed"])) == {0, 2}
    assert not r["p3p_req_out"]
    r = got["ok_p3p"]
    assert r["ran_p3p"] and r["p3p"]["status"] == 0 and (r["removed"] == 1).sum() == r["n_removed_p3p"] > 0 and not r["p3p_req_out"]
    assert (r["removed"] == 2).sum() == r["n_outliers_pnp"]
    r = got["ok_clean"]
    assert r["passes"][0]["ran"] and not r["passes"][1]["ran"] and not r["removed"].any()
    r = got["ok_no_l2"]
    assert not r["passes"][1]["ran"] and (r["removed"] == 2).sum() == r["n_outliers_pnp"] > 0
    # PNP_REQ_P3P: more than half of the blocks are outliers; nothing is removed, the pose stays, P3P is asked for
    params, pb, r = R.named_scene(oracle, "req_p3p")
    assert r["n_outliers_pnp"] > 0.5 * len(pb["unpx"]) and r["p3p_req_out"] and not r["removed"].any() and np.array_equal(r["Twc"], pb["Twc"])
    # P3P_RESET: fewer than 5 inliers with a model, and no valid row at all; the pose stays
    r = got["p3p_reset_few"]
    assert r["p3p"]["best_row"] >= 0 and r["p3p"]["status"] & p3p_ref.FEW_INLIERS and not r["passes"][0]["ran"]
    r = got["p3p_reset_no_row"]
    assert r["p3p"]["best_row"] == -1 and r["p3p"]["status"] == (p3p_ref.NO_MODEL | p3p_ref.FEW_INLIERS) and r["p3p"]["iterations"] == 0
    # PNP_RESET (mono) and PNP_KEEP (stereo) on the same data: P3P's pose and removals stand, PnP's do not, the flag is the input's
    (pm, pbm, rm), (ps, pbs, rs) = R.named_scene(oracle, "pnp_reset_mono"), R.named_scene(oracle, "pnp_keep_stereo")
    assert np.array_equal(pbm["unpx"], pbs["unpx"]) and np.array_equal(pbm["samples"], pbs["samples"])
    assert rm["action"] == R.PNP_RESET and rs["action"] == R.PNP_KEEP
    for r in (rm, rs):
        assert r["p3p"]["status"] == 0 and r["passes"][0]["ran"] and not (r["removed"] == 2).any() and r["p3p_req_out"] is True
        assert (r["removed"] == 1).sum() == r["n_removed_p3p"]
    assert np.array_equal(rm["Twc"], rs["Twc"]) and not np.array_equal(rm["Twc"], pbm["Twc"])
    # ceresPnP returns false because every block is bad (all points behind the camera)
    params, pb, r = R.named_scene(oracle, "all_behind")
    sub = R.ceres_pnp(oracle, pb)
    assert not sub["success"] and len(sub["outliers"]) == len(pb["unpx"]) and not sub["passes"][1]["ran"]
    assert r["action"] == R.PNP_REQ_P3P and r["p3p_req_out"]


@pytest.mark.parametrize("name", list(R.SCENES))
def test_named_scenes_meet_the_margin_conditions(oracle, name):
    params, pb, ref = R.named_scene(oracle, name)
    c = ref["chi2_pass1"][np.isfinite(ref["chi2_pass1"])]
    if len(c):
        print(name, "M1", np.min(np.abs(c - R.CHI2TH)) / R.CHI2TH)
        assert np.min(np.abs(c - R.CHI2TH)) > R.M1 * R.CHI2TH
    print(name, "M2", ref["p3p_th_margin"], "M3", ref["p3p_gap"])
    assert ref["p3p_th_margin"] > R.M2 and ref["p3p_gap"] > R.M3


@pytest.mark.parametrize("n", [4, 5, 63, 64, 65, 257, 308])
def test_pnp_cases_meet_the_margin_condition(oracle, n):
    for with_outliers in (False, True):
        for use_robust in (True, False):
            for apply_l2 in (True, False):
                pb, ref = R.pnp_case(oracle, n, with_outliers, use_robust, apply_l2)
                c = ref["chi2_pass1"][np.isfinite(ref["chi2_pass1"])]
                assert len(c) == n and np.min(np.abs(c - R.CHI2TH)) > R.M1 * R.CHI2TH
                assert ref["passes"][0]["ran"]
                assert ref["passes"][1]["ran"] == bool(apply_l2 and 0 < len(ref["outliers"]) < n)


def test_pose_from_model_is_a_unit_quaternion_of_the_rotation():
    rng = np.random.default_rng(5)
    for _ in range(50):
        Rm = R._so3_exp(rng.normal(0, 2.0, 3))
        p = R.pose_from_model(np.concatenate([Rm.reshape(9), [1.0, 2.0, 3.0]]))
        x, y, z, w = p[3:]
        back = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                         [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                         [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
        assert np.allclose(back, Rm, atol=1e-12) and np.array_equal(p[:3], [1.0, 2.0, 3.0])
