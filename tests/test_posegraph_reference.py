"""The specification of the pose-graph solver (tests/posegraph_ref.py) against THE REFERENCE'S OWN CODE and against itself:
LeftSE3RelativePoseError::Evaluate and SE3LeftParameterization through oracle/_ref/libref_factors.so (the reference's
src/ceres_parametrization.cpp compiled unchanged, see tests/test_reference_factors.py; tolerance 1e-11 relative for the same reason
as there: the stand-in headers evaluate the reference's expressions with plain loops), the block-tridiagonal solve against
numpy.linalg.solve on the dense matrix, the radius rules against the Ceres known answer that tests/test_oracle_ba.py uses, and the
two problem builders against the edge lists of the two call sites on a toy map."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import posegraph_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_SO = os.path.join(ROOT, "oracle", "_ref", "libref_factors.so")
RTOL = 1e-11


@pytest.fixture(scope="module")
def ref():
    if os.path.isdir("/root/reference"):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle", "ref")])
    if not os.path.exists(REF_SO):
        pytest.skip("oracle/_ref/libref_factors.so is absent and /root/reference is not here to build it from")
    return C.CDLL(REF_SO)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _rand_pose(rng, t_scale=1.0, rot=0.4):
    w = rng.normal(0, rot, 3)
    th = np.linalg.norm(w)
    return np.concatenate([rng.normal(0, t_scale, 3), np.sin(th / 2) * w / th, [np.cos(th / 2)]])


def _close(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max()) <= RTOL * max(1.0, float(np.abs(b).max()))


def _pairs():
    """200 (Twc0, Twc1, Tc0c1, sigma): generic errors, errors below 1e-9 rad (Sophus' small-angle branches), exactly zero, near pi"""
    rng = np.random.default_rng(21)
    out = []
    for k in range(200):
        P0, P1 = _rand_pose(rng, 3.0), _rand_pose(rng, 3.0)
        M = R.mul_pose(R.inv_pose(P0), P1)                         # zero error up to rounding
        if k % 4 == 0:
            M = R.mul_pose(M, _rand_pose(rng, 0.3, 0.3))
        elif k % 4 == 1:
            M = R.mul_pose(M, _rand_pose(rng, 1e-11, 1e-11))        # below 1e-10: both small-angle branches
        elif k % 4 == 2:
            ax = rng.normal(0, 1, 3); ax /= np.linalg.norm(ax)
            ang = np.pi - 10.0 ** rng.uniform(-9, -1)
            M = R.mul_pose(M, np.concatenate([rng.normal(0, 1, 3), np.sin(ang / 2) * ax, [np.cos(ang / 2)]]))
        out.append((P0, P1, M, (1.0, 0.5, 3.0)[k % 3]))
    return out


def test_factor_matches_the_reference(ref):
    worst = 0.0
    for P0, P1, M, sigma in _pairs():
        r = np.full(6, np.nan); J0 = np.full((6, 7), np.nan); J1 = np.full((6, 7), np.nan); chi2 = C.c_double(0)
        pp = (C.c_void_p * 2)(P0.ctypes.data, P1.ctypes.data); jj = (C.c_void_p * 2)(J0.ctypes.data, J1.ctypes.data)
        assert ref.ref_relpose_eval(_p(M), C.c_double(sigma), pp, _p(r), jj, C.byref(chi2)) == 0
        rs, A, B = R.edge_eval(P0[None], P1[None], M[None], np.array([1.0 / sigma]))
        assert _close(rs[0], r) and _close(A[0], J0[:, :6]) and _close(B[0], J1[:, :6]), (P0, P1, M)
        assert not J0[:, 6].any() and not J1[:, 6].any()            # 6x7 with a zero seventh column
        assert abs(float((rs[0] ** 2).sum()) - chi2.value) <= RTOL * max(1.0, chi2.value)
        # residual only (jacobians == NULL)
        r2 = np.full(6, np.nan)
        assert ref.ref_relpose_eval(_p(M), C.c_double(sigma), pp, _p(r2), None, C.byref(chi2)) == 0
        assert _close(R.edge_eval(P0[None], P1[None], M[None], np.array([1.0 / sigma]), jac=False)[0][0], r2)
        for a, b in ((rs[0], r), (A[0], J0[:, :6]), (B[0], J1[:, :6])):
            worst = max(worst, float(np.abs(a - b).max()) / max(1.0, float(np.abs(b).max())))
    print("largest relative difference %.3g" % worst)


def test_longdouble_factor_agrees_with_float64():
    for P0, P1, M, sigma in _pairs()[:40]:
        a = R.edge_eval(P0[None], P1[None], M[None], np.array([1.0 / sigma]))
        b = R.edge_eval(P0[None].astype(np.longdouble), P1[None].astype(np.longdouble), M[None].astype(np.longdouble),
                        np.array([1.0 / sigma], np.longdouble))
        assert b[0].dtype == np.longdouble
        for x, y in zip(a, b):
            assert float(np.abs(x - y).max()) <= 1e-9 * max(1.0, float(np.abs(x).max()))     # (near pi the log is ill-conditioned)


def test_plus_and_parameterisation_jacobian_match_the_reference(ref):
    rng = np.random.default_rng(22)
    for k in range(200):
        x = _rand_pose(rng, 3.0, 1.0)
        d = np.concatenate([rng.normal(0, 0.5, 3), rng.normal(0, (0.5, 1e-11, 3.0, 0.0)[k % 4], 3)])
        out = np.full(7, np.nan)
        assert ref.ref_se3_plus(_p(x), _p(d), _p(out)) == 0
        assert _close(R.plus(x[None], d[None])[0], out), (x, d)
        J = np.full(42, np.nan)
        assert ref.ref_se3_plus_jacobian(_p(x), _p(J)) == 0
        # [I6; 0]: the local Jacobians are the first six columns of the factor's blocks, which is what edge_eval returns
        assert np.array_equal(J.reshape(7, 6), np.vstack([np.eye(6), np.zeros((1, 6))]))


@pytest.mark.parametrize("n", [1, 2, 7, 65])
def test_block_tridiagonal_solve_matches_the_dense_solve(n):
    rng = np.random.default_rng(30 + n)
    G = rng.normal(0, 1, (n + 1, 12, 6))
    # a chain of Gauss-Newton blocks: SPD, block-tridiagonal; two breaks make three segments
    A = np.zeros((n, 6, 6)); Cc = np.zeros((n, 6, 6))
    breaks = {n // 3, 2 * n // 3} - {0} if n > 2 else set()
    for k in range(n):
        A[k] += G[k, :6].T @ G[k, :6] + 0.1 * np.eye(6)
        if k + 1 < n and (k + 1) not in breaks:
            A[k] += G[k, 6:].T @ G[k, 6:]; A[k + 1] += G[k + 1, :6].T @ G[k + 1, :6] * 0.5
            Cc[k] = G[k, 6:].T @ (G[k + 1, :6] * 0.5 ** 0.5)
    b = rng.normal(0, 1, (n, 6))
    cuts = [0] + sorted(breaks) + [n]
    segs = [(cuts[i], cuts[i + 1]) for i in range(len(cuts) - 1)]
    D = np.zeros((6 * n, 6 * n))
    for k in range(n):
        D[6 * k:6 * k + 6, 6 * k:6 * k + 6] = A[k]
        if k + 1 < n:
            D[6 * k:6 * k + 6, 6 * k + 6:6 * k + 12] = Cc[k]; D[6 * k + 6:6 * k + 12, 6 * k:6 * k + 6] = Cc[k].T
    want = np.linalg.solve(D, b.ravel()).reshape(n, 6)
    for dt in (np.float64, np.longdouble):
        y = R.block_tridiagonal_solve(A.astype(dt), Cc.astype(dt), b.astype(dt), segs)
        assert y.dtype == dt
        assert np.abs(y - want).max() <= 1e-9 * np.abs(want).max()
    A[n // 2] -= 1e3 * np.eye(6)
    assert R.block_tridiagonal_solve(A, Cc, b, segs) is None       # a non-positive pivot is a failed solve


def test_lm_radius_rules_give_the_ceres_known_answer():
    """AcceptRejectStepRadiusScaling (Ceres' levenberg_marquardt_strategy_test.cc:81-111), the sequence tests/test_oracle_ba.py
    holds the oracle to, through the two functions the specification's loop calls; exact equality"""
    seq = R.lm_radius_sequence(2.0, 20.0, [("reject", 0.0), ("reject", -1.0), ("accept", 1.0), ("accept", 1.0),
                                           ("accept", 0.25), ("accept", 1.0), ("accept", 1.0), ("accept", 1.0)])
    assert seq == [1.0, 0.25, 0.25 * 3.0, 0.25 * 3.0 * 3.0, 0.25 * 3.0 * 3.0 / 1.125,
                   0.25 * 3.0 * 3.0 / 1.125 * 3.0, 0.25 * 3.0 * 3.0 / 1.125 * 3.0 * 3.0, 20.0]


def _toy_map():
    rng = np.random.default_rng(40)
    return [_rand_pose(rng, 5.0) for _ in range(6)]


def test_local_builder_reproduces_the_call_site():
    """src/optimizer.cpp:2373-2424 on a toy map: keyframe ids 10 .. 15 with id 12 missing (:2391-2396) -- the chain skips it and
    its edge measures 11 -> 13; the loop edge goes from the loop keyframe to the new one, last"""
    from ov2slam_amd import optimizer as O
    kfs = _toy_map()
    loop = _rand_pose(np.random.default_rng(41))
    with_gap = list(kfs); with_gap[2] = None
    for build in (R.local_pose_graph, O.local_pose_graph_problem):
        p = build(with_gap, loop)
        assert p["edge_i"].tolist() == [0, 1, 2, 3, 0] and p["edge_j"].tolist() == [1, 2, 3, 4, 4]
        assert p["pose_const"].tolist() == [1, 0, 0, 0, 0]
        present = [kfs[k] for k in (0, 1, 3, 4, 5)]
        assert np.array_equal(p["poses"], np.array(present))
        for e in range(4):
            assert _close(p["edge_T"][e], R.mul_pose(R.inv_pose(present[e]), present[e + 1]))
            # the measurement is the current relative pose: the chain residuals vanish at the start
            r, _, _ = R.edge_eval(present[e][None], present[e + 1][None], p["edge_T"][e][None], np.ones(1), jac=False)
            assert np.abs(r).max() < 1e-13
        assert np.array_equal(p["edge_T"][4], loop)
        no_new = list(kfs); no_new[-1] = None
        assert build(no_new, loop) is None                          # :2392-2393: the reference returns false
    two = R.local_pose_graph(kfs[:2], loop)                         # two poses: the chain edge and the loop edge are the same pair
    assert two["edge_i"].tolist() == [0, 0] and two["edge_j"].tolist() == [1, 1]


def test_full_builder_reproduces_the_call_site():
    """src/optimizer.cpp:2794-2814: every frame a pose, keyframes constant, edge (i - 1, i) measuring vTpc[i]"""
    from ov2slam_amd import optimizer as O
    kfs = np.array(_toy_map())
    rng = np.random.default_rng(42)
    vTpc = np.array([_rand_pose(rng) for _ in range(6)])
    iskf = [True, False, False, True, True, False]
    for build in (R.full_pose_graph, O.full_pose_graph_problem):
        p = build(kfs, vTpc, iskf)
        assert p["edge_i"].tolist() == [0, 1, 2, 3, 4] and p["edge_j"].tolist() == [1, 2, 3, 4, 5]
        assert p["pose_const"].tolist() == [1, 0, 0, 1, 1, 0]
        assert np.array_equal(p["edge_T"], vTpc[1:]) and np.array_equal(p["poses"], kfs)
    S = R.Structure(R.full_pose_graph(kfs, vTpc, iskf))
    assert S.act.tolist() == [0, 1, 2, 4]                           # the edge between the two keyframes 3 and 4 takes no part
    assert S.segments == [(0, 2), (2, 3)]


def test_specification_solves_a_small_loop():
    """the loop on a 17-keyframe scene: the cost falls by orders of magnitude, float64 and longdouble decide alike, and a loop
    measurement 30 m / 3 rad off makes it reject steps"""
    p = R.make_local_scene(np.random.default_rng(117), 17)
    a, b = R.solve(p), R.solve(p, dt=np.longdouble)
    assert a["decisions"] == b["decisions"] and a["termination"] == R.TERM_FUNCTION_TOL and set(a["decisions"][:-1]) == {"o"}
    assert a["final_cost"] < 1e-2 * a["initial_cost"] and np.abs(a["poses"] - b["poses"]).max() < 1e-12
    assert np.array_equal(a["poses"][0], p["poses"][0])
    far = R.solve(R.make_local_scene(np.random.default_rng(24), 17, loop_far=True))
    assert "r" in far["decisions"]
    assert len(a["trace"]) == a["iterations"]                       # entry 0 + one per iteration, the one that ended inside the loop missing


def test_denormal_radius_fails_every_solve():
    """R.DENORMAL_RADIUS: five invalid steps, TERM_FAILURE, the input poses returned.  This case is EXEMPT from "float64 and longdouble
    decide alike" (tests/test_gpu_posegraph.py's condition): diag / radius = 1e304 overflows in float64 only, the longdouble run takes
    ordinary steps.  Only decisions and copied values are compared on it."""
    p = R.denormal_radius_scene()
    a = R.solve(p, R.options(**R.DENORMAL_RADIUS))
    print("float64: %s, %d iterations, termination %d" % (a["decisions"], a["iterations"], a["termination"]))
    assert a["decisions"] == "iiiiix" and a["termination"] == R.TERM_FAILURE and a["iterations"] == 5 and a["num_successful_steps"] == 1
    assert np.array_equal(a["poses"], p["poses"]) and a["final_cost"] == a["initial_cost"] > 0
    assert [t["trust_region_radius"] for t in a["trace"]] == [1e-310, 1e-310 / 2, 1e-310 / 2 / 4, 1e-310 / 2 / 4 / 8, 1e-310 / 2 / 4 / 8 / 16]
    assert all(not t["step_is_valid"] and t["cost"] == a["initial_cost"] for t in a["trace"][1:])
    b = R.solve(p, R.options(**R.DENORMAL_RADIUS), dt=np.longdouble)
    assert "i" not in b["decisions"] and b["termination"] != R.TERM_FAILURE            # (why the case is exempt)
    # the invalid budget, the radius floor (9.765625e-314 <= 1e-312 after four invalid steps) and the iteration budget inside the run
    two = R.solve(p, R.options(**dict(R.DENORMAL_RADIUS, max_consecutive_invalid_steps=2)))
    assert two["decisions"] == "iix" and two["termination"] == R.TERM_FAILURE and two["iterations"] == 2
    floor = R.solve(p, R.options(**dict(R.DENORMAL_RADIUS, min_radius=1e-312)))
    assert floor["decisions"] == "iiiis" and floor["termination"] == R.TERM_MIN_RADIUS and floor["iterations"] == 4
    budget = R.solve(p, R.options(**dict(R.DENORMAL_RADIUS, max_iter=3)))
    assert budget["decisions"] == "iiim" and budget["termination"] == R.TERM_NO_CONVERGENCE and budget["iterations"] == 3
    for r in (two, floor, budget):
        assert np.array_equal(r["poses"], p["poses"]) and r["final_cost"] == r["initial_cost"]
