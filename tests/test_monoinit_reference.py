"""The numpy specification of the device mono initialisation chain (tests/monoinit_ref.py) on its own: the named scenes reach every
action and each side of every comparison, and they satisfy the CONDITIONS under which the device is compared with the specification
bit for bit (tests/test_gpu_monoinit.py), which are those of tests/test_epifilter_reference.py:
  - no row that float64 and long double decide differently (fivept_ref.fragile_rows) lies among the rows the loop consumes;
  - no distance of the winning model lies within a relative 1e-9 of its threshold;
  - p0 and p1 are not within a relative 1e-6 of finit_parallax, except in the boundary scenes, which are built from exactly
    representable inputs;
and the two restatements of the file agree with their matrix forms in float64: K rotbv with K @ R @ bv to 1e-12 relative, Twc_init
is a unit quaternion behind a translation of length 0.25 to 1e-15.  These are conditions on the seeds, checked here without a
device."""
import numpy as np
import pytest

from tests import epifilter_ref as EF
from tests import fivept_ref as E5
from tests import kfreq_ref as KF
from tests import monoinit_ref as R
from tests.tri_ref import D, matvec


def _all():
    return {n: R.expected(n, True) for n in R.SCENE_NAMES}


def test_scenes_reach_every_action_and_each_side_of_every_comparison():
    E = _all()
    assert {e["action"] for e in E.values()} == set(R.ACTIONS)
    act = lambda n: E[n]["action"]
    # :100
    a, b = E["nb2dkps_49"], E["nb2dkps_50"]
    assert (a["nb2dkps"], a["action"], b["nb2dkps"]) == (49, R.RESET, 50) and b["action"] != R.RESET
    assert R.scene("nb2dkps_49")[0]["min_2d_kps"] == 50 and all(R.scene(n)[0]["min_2d_kps"] == 0 for n in R.SCENE_NAMES if "nb2dkps" not in n)
    assert a["p0_n"] == 0 and float(a["p0"]) == 0.0 and not a["removed"].any()                 # nothing else ran
    # :861, strict: equality does not pass
    assert float(E["p0_below"]["p0"]) < 20.0 == float(E["p0_at"]["p0"]) < float(E["p0_above"]["p0"])
    assert act("p0_below") == act("p0_at") == R.LOW_PARALLAX and act("p0_above") == R.NO_MODEL
    assert act("n_kf_0") == R.LOW_PARALLAX and float(E["n_kf_0"]["p0"]) == 0.0 and E["n_kf_0"]["p0_n"] == 0
    assert R.scene("n_kf_0")[2]["kps"] == {}
    # :873, :917
    assert act("n_cur_7") == R.TOO_FEW_KPS and act("n_cur_8") not in (R.TOO_FEW_KPS, R.LOW_PARALLAX)
    assert (E["m_7_of_12"]["m"], act("m_7_of_12")) == (7, R.TOO_FEW_MATCHES) and float(E["m_7_of_12"]["p1"]) == 0.0
    assert E["m_8_of_12"]["m"] == 8 and E["m_8_of_12"]["rows_consumed"] > 0                    # searched: eight matches are enough
    # :925, strict the other way: equality passes
    assert float(E["p1_below"]["p1"]) == 20.0 - 2.0 ** -13 and float(E["p1_at"]["p1"]) == 20.0 and float(E["p1_above"]["p1"]) == 20.0 + 2.0 ** -13
    assert act("p1_below") == R.LOW_ROT_PARALLAX and act("p1_at") == act("p1_above") == R.NO_MODEL
    assert E["p1_at"]["search"] is not None and E["p1_below"]["search"] is None
    # the case the second gate exists for
    e, P = E["rotation_only"], R.scene("rotation_only")[0]
    assert act("rotation_only") == R.LOW_ROT_PARALLAX and float(e["p0"]) > 3 * P["fkf"]["finit_parallax"] and float(e["p1"]) < 1.0
    # :956
    assert E["inliers_9"]["n_inliers"] == 9 and E["inliers_9"]["status"] == E5.FEW_INLIERS and act("inliers_9") == R.NO_MODEL
    assert not E["inliers_9"]["removed"].any() and E["inliers_9"]["n_outliers"] == 1 and E["inliers_9"]["n_removed"] == 0
    assert E["inliers_10"]["n_inliers"] == 10 and act("inliers_10") == R.READY
    # :962: no 50 % rule
    e = E["mismatches_30_percent"]
    assert e["action"] == R.READY and e["m"] == 60 and e["n_outliers"] == e["n_removed"] == 18 == int(e["removed"].sum())
    e = E["outliers_over_half"]
    assert e["action"] == R.READY and e["n_outliers"] > 0.5 * e["m"] and e["n_removed"] == e["n_outliers"] == int(e["removed"].sum())
    assert np.array_equal(np.nonzero(e["removed"])[0], np.sort(e["pair_cur"][e["search"]["outliers"]]))
    for ax in "wxyz":
        e = E["quat_%s" % ax]
        assert e["action"] == R.READY and EF.quat_branch(e["model"]) == ax
    for n, size, rows in (("size_63_rows_1", 63, 1), ("size_64_rows_64", 64, 64), ("size_65_rows_65", 65, 65), ("size_308_rows_200", 308, 200)):
        assert len(R.scene(n)[1]["kps"]) == size and R.scene(n)[0]["n_rows"] == rows and len(E[n]["samples"]) == rows
        assert act(n) == R.READY and 0 < E[n]["n_removed"] < E[n]["m"] < size                  # some ids the keyframe does not hold
    for e in E.values():
        assert e["pose_refined"] == 0 and bool(e["Twc_init"].any()) == (e["action"] == R.READY)


@pytest.mark.parametrize("name", R.SCENE_NAMES)
def test_no_fragile_row_is_consumed_and_nothing_sits_on_a_threshold(name):
    P, cur, kf = R.scene(name)
    e = R.expected(name, True)
    finit = float(np.float32(P["fkf"]["finit_parallax"]))
    if name not in R.ON_BOUNDARY:
        if e["action"] != R.RESET:
            assert abs(float(e["p0"]) - finit) > 1e-6 * finit, "p0 within 1e-6 of finit_parallax"
        if e["action"] >= R.LOW_ROT_PARALLAX:
            assert abs(float(e["p1"]) - finit) > 1e-6 * finit, "p1 within 1e-6 of finit_parallax"
    s = e["search"]
    if s is None:
        return
    consumed = np.asarray(s["consumed_rows"], np.int64)
    assert not e["fragile"][consumed].any(), "a fragile row among the rows the loop consumes: choose another seed"
    if s["best_row"] >= 0:
        th = P["threshold"]
        d = e["prep"][1][s["best_row"]]
        assert np.all(np.abs(d - th) > 1e-9 * th), "a distance of the winning model within 1e-9 of the threshold"


@pytest.mark.parametrize("name", R.SCENE_NAMES)
def test_restated_parallax_and_pose_agree_with_their_matrix_forms(name):
    P, cur, kf = R.scene(name)
    e = R.expected(name, True)
    fx, fy, cx, cy = P["fkf"]["K"]
    K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]])
    Rm = KF.rkfcur(kf["Tcw"], cur["Twc"])
    Rn = np.array(Rm, np.float64)
    for kp in cur["kps"].values():
        got = np.array(R.k_times(P["fkf"]["K"], matvec(Rm, tuple(D(c) for c in kp["bv"]))), np.float64)
        want = K @ Rn @ np.asarray(kp["bv"], np.float64)
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    if e["action"] != R.READY:
        return
    T = e["Twc_init"]
    assert abs(np.sqrt((T[3:] ** 2).sum()) - 1.0) <= 1e-15 and abs(np.sqrt((T[:3] ** 2).sum()) - 0.25) <= 1e-15
    t = e["model"][9:]
    assert np.abs(T[:3] - 0.25 * t / np.linalg.norm(t)).max() <= 1e-15
    # the quaternion is the model's rotation
    x, y, z, w = T[3:]
    Rq = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                   [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                   [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    assert np.abs(Rq - e["model"][:9].reshape(3, 3)).max() <= 1e-12


def test_flat_item_gives_the_same_p0():
    """the device computes p0 on the flattened item (kfreq_ref.flat_parallax is k_fkf_parallax's form): the same bits as the loop"""
    for name in R.SCENE_NAMES:
        P, cur, kf = R.scene(name)
        e = R.expected(name, True)
        if e["action"] == R.RESET:
            continue
        f = KF.flat_parallax(P["fkf"], R.flatten(cur, kf), 0, KF.ALL, KF.MEDIAN)
        assert (KF.bits(f["parallax"]), f["n"], f["n_distinct"], f["n_nonfinite"]) == \
               (KF.bits(e["p0"]), e["p0_n"], e["p0_n_distinct"], e["p0_n_nonfinite"]), name
