"""tests/ba_cases.py is what tests/test_gpu_ba_structure.py stands on: the structure it promises is checked here, and so is -- on the
oracle alone, no GPU -- that its problems are well posed enough for the device bar (1e-7, identical decisions) to mean something:
the oracle against itself on two block orders of one problem stays 100x under that bar."""
import numpy as np
import pytest

import ov2slam_amd
from tests import ba_cases as B

OPTION_SETS = (dict(), dict(max_iter=10, huber_delta=-1.0), dict(max_iter=12, function_tolerance=1e-9))
ORDER_TOL = 1e-9                  # two block orders on the oracle: 100x under the device bar
TH = 5.9915


@pytest.fixture(scope="module")
def irregular():
    return B.irregular_invdepth(), B.irregular_invdepth(shuffle=False)


def _has_run(counts, anchors, pattern):
    """eight consecutive landmarks (in anchor order: a stable sort by anchor keyframe) of one anchor with these counts, in this
    order or, for an alternating pattern, starting with either value"""
    order = np.argsort(anchors, kind="stable")
    c, a = counts[order], anchors[order]
    n = len(pattern)
    for i in range(len(c) - n + 1):
        if np.all(a[i:i + n] == a[i]) and (list(c[i:i + n]) == list(pattern) or list(c[i:i + n]) == list(pattern[1:]) + [pattern[0]]):
            return True
    return False


def test_the_standard_layout_has_the_promised_structure(irregular):
    pb, ps = irregular
    counts, anchors = pb["counts"], pb["lm_anchor_kf"]
    assert np.array_equal(np.bincount(pb["res_lm"], minlength=pb["n_lm"]), counts)          # the counts are exact
    for name, pattern in B.RUN_PATTERNS.items():
        assert _has_run(counts, anchors, pattern), name
    assert (counts == 128).sum() >= 1 and (counts == 129).sum() >= 1 and (counts == 63).sum() >= 1 and (counts == 0).sum() >= 8
    assert not np.all(np.diff(anchors) >= 0)                                                  # landmark order is not anchor order
    # few anchors, at least one of them constant; constant keyframes at the start, in the middle and at the end
    used = np.unique(anchors)
    assert 2 <= len(used) <= 8 and pb["kf_const"][used].any() and not pb["kf_const"][used].all()
    const = np.nonzero(pb["kf_const"])[0]
    assert const[0] == 0 and const[-1] == pb["n_kf"] - 1 and np.any((const > 10) & (const < pb["n_kf"] - 10))
    # one free keyframe without any block, every other free keyframe observes at least 12
    seen = np.bincount(pb["res_kf"][pb["res_type"] != B.RIGHT_ANCH], minlength=pb["n_kf"])
    e = pb["empty_kf"]
    assert seen[e] == 0 and not pb["kf_const"][e] and e not in used
    free = np.nonzero(pb["kf_const"] == 0)[0]
    assert seen[free[free != e]].min() >= 12
    # RIGHT_ANCH on some landmarks only; stereo observers, left-only and right-only ones
    with_ra = np.bincount(ps["res_lm"][ps["res_type"] == B.RIGHT_ANCH], minlength=pb["n_lm"]) > 0
    assert with_ra[counts > 0].any() and not with_ra[counts > 0].all()
    key = ps["res_lm"].astype(np.int64) * pb["n_kf"] + ps["res_kf"]
    obs = ps["res_type"] != B.RIGHT_ANCH
    nl = np.bincount(key[obs & (ps["res_type"] == B.LEFT)], minlength=pb["n_lm"] * pb["n_kf"])
    nr = np.bincount(key[obs & (ps["res_type"] == B.RIGHT)], minlength=pb["n_lm"] * pb["n_kf"])
    assert nl.max() == 1 and nr.max() == 1
    n_both, n_lonly, n_ronly = int(((nl == 1) & (nr == 1)).sum()), int(((nl == 1) & (nr == 0)).sum()), int(((nl == 0) & (nr == 1)).sum())
    assert n_both > n_lonly + n_ronly and n_lonly > 20 and n_ronly > 20                       # most observers are stereo
    assert not np.any(ps["res_kf"][obs] == anchors[ps["res_lm"][obs]])                      # nobody observes from the anchor
    # weights, calibration, extrinsics
    assert set(np.round(np.log(pb["res_sigma"]) / np.log(1.2)).astype(int)) == {0, 1, 2, 3}
    assert np.abs(pb["calib_r"] - pb["calib_l"]).min() > 0.5
    angle = 2 * np.arccos(min(1.0, abs(pb["T_rl"][6])))
    assert np.deg2rad(0.3) < angle < np.deg2rad(0.8) and np.all(pb["T_rl"][3:6] != 0)
    # outliers: every block of the dead landmarks, a few percent elsewhere
    dead = pb["dead"]
    assert len(dead) >= 3 and set(counts[dead]) == {1, 2}
    on_dead = np.isin(ps["res_lm"], dead)
    assert ps["is_outlier"][on_dead].all() and 0.01 < ps["is_outlier"][~on_dead].mean() < 0.06
    # the block order: a permutation of the landmark-sorted problem, and not sorted itself
    perm = pb["perm"]
    assert np.array_equal(np.sort(perm), np.arange(pb["n_res"])) and np.all(np.diff(ps["res_lm"]) >= 0)
    assert (np.diff(pb["res_lm"]) < 0).sum() > pb["n_res"] // 4
    for k in ("res_type", "res_kf", "res_lm", "res_uv", "res_sigma"):
        assert np.array_equal(pb[k], ps[k][perm]), k
    assert np.array_equal(B.unshuffle(pb["res_uv"], perm), ps["res_uv"])


def test_the_other_forms_and_the_sweep_have_their_counts():
    for pb in (B.irregular_xyz(), B.irregular_structure()):
        assert np.array_equal(np.bincount(pb["res_pt"], minlength=pb["n_pts"]), pb["counts"])
        for c in B.XYZ_COUNTS:
            assert (pb["counts"] == c).sum() >= 3
        assert (np.diff(pb["res_pt"]) < 0).sum() > pb["n_res"] // 4
        assert not np.any(pb["res_kf"] == pb["empty_kf"]) and set(pb["res_type"]) == {0, 1}
    assert "kf_const" not in B.irregular_structure() and np.array_equal(B.irregular_structure()["poses"], B.irregular_structure()["poses_gt"])
    for c in B.SWEEP_COUNTS:
        pb = B.count_sweep_problem(c)
        assert pb["n_lm"] == 24 and np.all(np.bincount(pb["res_lm"], minlength=24) == c) and len(np.unique(pb["lm_anchor_kf"])) == 2
        assert pb["n_kf"] >= 10 and pb["kf_const"][0] == 1
    rng = np.random.default_rng(3)
    for _ in range(5):
        pb = B.random_case(rng)
        assert np.array_equal(np.bincount(pb["res_lm"], minlength=pb["n_lm"]), pb["counts"]) and pb["counts"].max() <= 140
        assert not np.any(pb["res_kf"][pb["res_type"] != B.RIGHT_ANCH] == pb["empty_kf"]) and pb["kf_const"].any()


def _same_decisions(a, b):
    return a["iterations"] == b["iterations"] and a["termination"] == b["termination"] and a["num_successful_steps"] == b["num_successful_steps"]


def _order_spread(a, b, perm, key):
    """largest parameter difference of two solves of one problem in two block orders (a: shuffled by perm); decisions must agree"""
    assert _same_decisions(a, b)
    ca = B.unshuffle(a["chi2"], perm)
    m = np.isfinite(b["chi2"])
    assert np.array_equal(np.isfinite(ca), m) and np.array_equal(ca[m] > TH, b["chi2"][m] > TH)
    assert np.array_equal(B.unshuffle(a["depthpos"], perm), b["depthpos"])
    d = float(np.abs(a[key] - b[key]).max())
    return max(d, float(np.abs(a["poses"] - b["poses"]).max())) if "poses" in a else d


def test_the_irregular_problem_is_well_posed_on_the_oracle(oracle, irregular, capsys):
    pb, ps = irregular
    spread = 0.0
    fixed = np.nonzero(pb["kf_const"])[0].tolist() + [pb["empty_kf"]]
    for kw in OPTION_SETS:
        r = oracle.ba_solve(pb, oracle.ba_default_options(**kw))
        assert r["termination"] == 1 and r["final_cost"] < 0.5 * r["initial_cost"], (kw, r["termination"])       # FUNCTION_TOLERANCE
        assert np.array_equal(r["poses"][fixed], pb["poses"][fixed])                # constant and empty keyframes: not one bit moves
        assert np.array_equal(r["invdepth"][pb["counts"] == 0], pb["invdepth"][pb["counts"] == 0])
        spread = max(spread, _order_spread(r, oracle.ba_solve(ps, oracle.ba_default_options(**kw)), pb["perm"], "invdepth"))

    def solver(prob, res_active, chi2_init, depthpos_init, **kw):
        return oracle.ba_solve(prob, oracle.ba_default_options(**kw), res_active, chi2_init, depthpos_init)
    la = ov2slam_amd.Optimizer(None, solver=solver).localBA(pb)
    lb = ov2slam_amd.Optimizer(None, solver=solver).localBA(ps)
    assert la["l2_done"] and lb["l2_done"]
    # landmarks that lose every block in pass 1: the dead ones, at least
    bad1 = la["bad_after_pass1"]
    lost = [l for l in range(pb["n_lm"]) if pb["counts"][l] > 0 and bad1[pb["res_lm"] == l].all()]
    assert len(lost) >= 3 and set(pb["dead"]) <= set(lost)
    assert np.array_equal(la["pass2"]["invdepth"][lost], la["pass1"]["invdepth"][lost])      # pass 2 leaves them where they are
    # no decision hangs on the last digits of a chi2
    margin = min(float(np.abs(p["chi2"][np.isfinite(p["chi2"])] - TH).min()) for p in (la["pass1"], la["pass2"]))
    assert margin > 1e-4, margin
    for k in ("bad_after_pass1", "bad_obs"):
        assert np.array_equal(B.unshuffle(la[k], pb["perm"]), lb[k]), k
    for q in ("pass1", "pass2"):
        spread = max(spread, _order_spread(la[q], lb[q], pb["perm"], "invdepth"))
    with capsys.disabled():
        print("\n  irregular problem (%d keyframes, %d landmarks, %d blocks): the oracle on two block orders differs by %.2e at most; "
              "%d landmarks lose every block in pass 1; nearest chi2 to the threshold: %.1e away" % (pb["n_kf"], pb["n_lm"], pb["n_res"], spread, len(lost), margin))
    assert spread <= ORDER_TOL, spread


def test_the_sweep_and_the_point_forms_are_well_posed_on_the_oracle(oracle, capsys):
    """the count sweep (every option set), the 3-D point form (the option sets tests/test_gpu_ba_structure.py uses) and the
    structure-only form: two block orders on the oracle, identical decisions, parameters within 1e-9"""
    worst = {}
    for c in B.SWEEP_COUNTS:
        pb = B.count_sweep_problem(c)
        ps = dict(pb)
        for k in pb:
            if k.startswith("res_"):
                ps[k] = B.unshuffle(pb[k], pb["perm"])
        for kw in OPTION_SETS:
            a, b = oracle.ba_solve(pb, oracle.ba_default_options(**kw)), oracle.ba_solve(ps, oracle.ba_default_options(**kw))
            assert a["termination"] in (0, 1) and a["final_cost"] < a["initial_cost"]
            worst["sweep"] = max(worst.get("sweep", 0.0), _order_spread(a, b, pb["perm"], "invdepth"))
    pb, ps = B.irregular_xyz(), B.irregular_xyz(shuffle=False)
    for kw in OPTION_SETS[:2]:
        a, b = oracle.xyz_ba_solve(pb, oracle.ba_default_options(**kw)), oracle.xyz_ba_solve(ps, oracle.ba_default_options(**kw))
        assert a["termination"] in (0, 1) and a["final_cost"] < a["initial_cost"]
        worst["xyz"] = max(worst.get("xyz", 0.0), _order_spread(a, b, pb["perm"], "xyz"))

    def solver(prob, res_active, chi2_init, depthpos_init, **kw):
        return oracle.xyz_ba_solve(prob, oracle.ba_default_options(**kw), res_active, chi2_init, depthpos_init)
    la, lb = ov2slam_amd.Optimizer(None, solver=solver).localBA(pb), ov2slam_amd.Optimizer(None, solver=solver).localBA(ps)
    assert la["l2_done"] and np.array_equal(B.unshuffle(la["bad_obs"], pb["perm"]), lb["bad_obs"])
    for l in pb["dead"]:
        assert la["bad_after_pass1"][pb["res_pt"] == l].all()
    assert min(float(np.abs(p["chi2"][np.isfinite(p["chi2"])] - TH).min()) for p in (la["pass1"], la["pass2"])) > 1e-4
    worst["xyz"] = max(worst["xyz"], _order_spread(la["pass1"], lb["pass1"], pb["perm"], "xyz"), _order_spread(la["pass2"], lb["pass2"], pb["perm"], "xyz"))
    pb, ps = B.irregular_structure(), B.irregular_structure(shuffle=False)
    for kw in (dict(max_iter=10, function_tolerance=1e-3, huber_delta=float(np.sqrt(TH))), dict(max_iter=30, function_tolerance=1e-9, huber_delta=-1.0)):
        a, b = oracle.structure_ba(pb, oracle.ba_default_options(**kw)), oracle.structure_ba(ps, oracle.ba_default_options(**kw))
        assert a["termination"] == 1
        worst["structure"] = max(worst.get("structure", 0.0), _order_spread(a, b, pb["perm"], "xyz"))
    with capsys.disabled():
        print("\n  the oracle on two block orders: " + ", ".join("%s %.2e" % kv for kv in worst.items()))
    assert max(worst.values()) <= ORDER_TOL, worst
