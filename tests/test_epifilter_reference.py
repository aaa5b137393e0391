"""The numpy specification of the device epipolar2d2dFiltering chain (tests/epifilter_ref.py) on its own: the named scenes reach
every action and every branch, and they satisfy the CONDITIONS under which the device is compared with the specification bit for
bit (tests/test_gpu_epifilter.py):
  - no row that float64 and long double decide differently (fivept_ref.fragile_rows) lies among the rows the loop consumes;
  - no distance of the winning model and no Sampson error lies within a relative 1e-9 of its threshold (the scenes built exactly
    on a boundary use exactly representable inputs instead and are exempt);
and the two restatements of the file agree with their matrix forms in float64: F with inv(K).T hat(t) R inv(K) to 1e-12 relative,
the mono pose (a unit quaternion) with the product of the 4 x 4 matrices to 1e-12.  These are conditions on the seeds, checked
here without a device."""
import numpy as np
import pytest

from tests import epifilter_ref as R
from tests import fivept_ref as E5
from tests.tri_ref import rotation_matrix


def _all():
    return {n: R.expected(n, True) for n in R.SCENE_NAMES}


def test_scenes_reach_every_action_and_branch():
    E = _all()
    assert {e["action"] for e in E.values()} == {R.TOO_FEW_KPS, R.LOW_PARALLAX, R.NO_MODEL, R.DEGENERATE, R.FILTERED}
    act = lambda n: E[n]["action"]
    assert act("n_cur_7") == R.TOO_FEW_KPS and act("n_cur_8") != R.TOO_FEW_KPS
    assert E["m_7_of_12"]["m"] == 7 and E["m_7_of_12"]["status"] == E5.TOO_FEW_POINTS and act("m_7_of_12") == R.NO_MODEL
    assert E["m_8_of_12"]["m"] == 8 and E["m_8_of_12"]["rows_consumed"] > 0        # searched: eight matches are enough
    for kind in ("given", "counted"):
        a, b = E["stereo_nb3d_30_%s" % kind], E["stereo_nb3d_31_%s" % kind]
        assert (a["nb3dkps"], a["epifrom3dkps"], b["nb3dkps"], b["epifrom3dkps"]) == (30, 0, 31, 1)
        assert a["m"] == 64 and b["m"] == 31 and not a["F"].any() and b["F"].any()
    assert act("gate_below") == R.LOW_PARALLAX and act("gate_at") == R.NO_MODEL and act("gate_above") == R.NO_MODEL
    assert float(E["gate_below"]["parallax"]) < 6.0 == float(E["gate_at"]["parallax"]) < float(E["gate_above"]["parallax"])
    for n in ("m_0_nan_parallax", "n_kf_0"):
        assert E[n]["m"] == 0 and np.isnan(E[n]["parallax"]) and act(n) == R.NO_MODEL and E[n]["status"] == E5.TOO_FEW_POINTS
    assert R.scene("n_kf_0")[2]["kps"] == {} and R.scene("m_0_nan_parallax")[2]["kps"]
    assert E["inliers_9"]["n_inliers"] == 9 and E["inliers_9"]["status"] == E5.FEW_INLIERS and act("inliers_9") == R.NO_MODEL
    assert E["inliers_10"]["n_inliers"] == 10 and act("inliers_10") == R.FILTERED
    a, b = E["outliers_half"], E["outliers_half_plus_1"]
    assert a["m"] == b["m"] == 60 and a["n_outliers"] == 30 and b["n_outliers"] == 31         # m / 2 and m / 2 + 1
    assert a["action"] == R.FILTERED and a["n_removed_ransac"] == 30 and b["action"] == R.DEGENERATE and not b["removed"].any()
    P, cur, kf = R.scene("stereo_2d_unknown_to_keyframe")
    e = E["stereo_2d_unknown_to_keyframe"]
    absent2d = [i for i, k in enumerate(cur["kps"].values()) if not k["is3d"] and k["lmid"] not in kf["kps"]]
    assert absent2d and e["epifrom3dkps"] and all(e["err"][i] > 0 for i in absent2d)       # scored against (0, 0), not skipped
    assert (e["removed"] == 1).any() and (e["removed"] == 2).any()
    for nbkfs in (2, 3):
        for nb in (29, 30):
            e = E["mono_nbkfs_%d_nb3d_%d" % (nbkfs, nb)]
            want = int(nbkfs > 2 and nb < 30)
            assert e["action"] == R.FILTERED and (e["do_optimize"], e["pose_from_model"]) == (want, want)
            assert bool(e["Twc_model"].any()) == bool(want)
    for ax in "wxyz":
        a, b = E["mono_quat_%s" % ax], E["stereo_quat_%s" % ax]
        assert a["action"] == b["action"] == R.FILTERED and R.quat_branch(a["model"]) == R.quat_branch(b["model"]) == ax
        assert a["pose_from_model"] == 1 and b["epifrom3dkps"] == 1 and b["n_removed_sampson"] > 0
    for n, size, rows in (("size_63_rows_1", 63, 1), ("size_64_rows_64", 64, 64), ("size_65_rows_65", 65, 65), ("size_308_rows_200", 308, 200)):
        assert len(R.scene(n)[1]["kps"]) == size and R.scene(n)[0]["n_rows"] == rows and len(E[n]["samples"]) == rows


@pytest.mark.parametrize("name", R.SCENE_NAMES)
def test_no_fragile_row_is_consumed_and_nothing_sits_on_a_threshold(name):
    P, cur, kf = R.scene(name)
    e = R.expected(name, True)
    s = e["search"]
    if s is None or e["m"] < 8:
        return
    consumed = np.asarray(s["consumed_rows"], np.int64)
    assert not e["fragile"][consumed].any(), "a fragile row among the rows the loop consumes: choose another seed"
    if name in R.ON_BOUNDARY:
        return
    th = P["threshold"]
    if s["best_row"] >= 0:
        d = e["prep"][1][s["best_row"]]
        assert np.all(np.abs(d - th) > 1e-9 * th), "a distance of the winning model within 1e-9 of the threshold"
    if e["action"] == R.FILTERED and e["epifrom3dkps"]:
        is2d = np.array([not k["is3d"] for k in cur["kps"].values()])
        err = e["err"][is2d].astype(np.float64)
        assert np.all(np.abs(err - P["fransac_err"]) > 1e-9 * P["fransac_err"]), "a Sampson error within 1e-9 of fransac_err"


@pytest.mark.parametrize("name", R.SCENE_NAMES)
def test_restated_F_and_mono_pose_agree_with_their_matrix_forms(name):
    P, cur, kf = R.scene(name)
    e = R.expected(name, True)
    if e["best_row"] < 0:
        return
    model = e["model"]
    fx, fy, cx, cy = P["fkf"]["K"]
    K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]])
    Rm, t = model[:9].reshape(3, 3), model[9:]
    hat = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    iK = np.linalg.inv(K)
    want = iK.T @ hat @ Rm @ iK
    got = R.fundamental(P["fkf"]["K"], model).reshape(3, 3)
    # R' is the matrix of the QUATERNION of Rkfc: it equals Rkfc as far as the search's R is orthonormal, which it is to ~1e-15
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    T = R.mono_pose(kf["Twc"], kf["Tcw"], cur["Twc"], model)
    assert abs(np.sqrt((T[3:] ** 2).sum()) - 1.0) <= 1e-12

    def mat(p):
        M = np.eye(4)
        M[:3, :3] = np.array(rotation_matrix(tuple(p[3:7])), np.float64)
        M[:3, 3] = p[:3]
        return M
    scale = np.linalg.norm((mat(np.asarray(kf["Tcw"])) @ mat(np.asarray(cur["Twc"])))[:3, 3])
    Tk = np.eye(4)
    Tk[:3, :3], Tk[:3, 3] = Rm, scale * t / np.linalg.norm(t)
    want = mat(np.asarray(kf["Twc"])) @ Tk
    assert np.abs(mat(T) - want).max() <= 1e-12 * max(1.0, np.abs(want).max())


def test_remove_lmids_order():
    """RANSAC outliers ascending in join order, then the 2-D ids in array order"""
    P, cur, kf = R.scene("stereo_2d_unknown_to_keyframe")
    e = R.expected("stereo_2d_unknown_to_keyframe", True)
    ids = [k["lmid"] for k in cur["kps"].values()]
    out = R.remove_lmids(cur, e)
    n1 = e["n_removed_ransac"]
    assert len(out) == n1 + e["n_removed_sampson"] and len(set(out)) == len(out)
    pos = [ids.index(v) for v in out]
    assert pos[:n1] == sorted(pos[:n1]) and pos[n1:] == sorted(pos[n1:])
    assert all(e["removed"][p] == 1 for p in pos[:n1]) and all(e["removed"][p] == 2 for p in pos[n1:])
