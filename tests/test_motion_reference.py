"""The specification of the motion model (tests/motion_ref.py) against the oracle and against itself: SE3::exp against the oracle's
orc_se3_exp (the oracle's C restatement of Sophus, pinned by tests/test_oracle_ba.py), exp and log as each other's inverse, the
branches of applyMotionModel and updateMotionModel, a constant-velocity trajectory reproduced by update followed by apply, and THE
CONDITION of tests/test_gpu_motion.py: on every committed case float64 and longdouble agree on `resynced` and no |d_k| lies within
1e-7 of the 1e-5 threshold."""
import ctypes as C

import numpy as np

from tests import motion_ref as M
from tests import posegraph_ref as R


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _tangents():
    """generic tangents, rotations below Sophus' small-angle switch (theta^2 < 1e-20), exactly zero, rotations of several radians"""
    rng = np.random.default_rng(41)
    out = []
    for k in range(120):
        a = np.concatenate([rng.normal(0, 1.0, 3), rng.normal(0, 0.7, 3)])
        if k % 4 == 1:
            a[3:] = rng.normal(0, 1e-11, 3)
        elif k % 4 == 2:
            a[3:] *= 4.0
        elif k % 12 == 3:
            a[3:] = 0.0
        out.append(a)
    return out


def test_exp_matches_the_oracle(oracle):
    worst, n_small = 0.0, 0
    for a in _tangents():
        t, q = np.full(3, np.nan), np.full(4, np.nan)
        oracle.lib().orc_se3_exp(_p(a), _p(t), _p(q))
        qe, te = M.exp(a)
        n_small += float((a[3:] ** 2).sum()) < 1e-20
        worst = max(worst, float(np.abs(qe[0] - q).max()), float(np.abs(te[0] - t).max() / max(1.0, np.abs(t).max())))
    print("largest difference %.3g, %d tangents below the small-angle switch" % (worst, n_small))
    assert n_small >= 30 and worst <= 1e-14


def test_log_of_exp_and_exp_of_log():
    for dt, tol in ((np.float64, 1e-12), (np.longdouble, 1e-15)):
        for a in _tangents():
            if np.linalg.norm(a[3:]) >= np.pi:                  # log returns the rotation vector within (-pi, pi)
                continue
            back = R.log(M.exp(a, dt))[0]
            # below the switch Sophus' exp takes V = R = I + hat(omega) where the series has I + hat(omega) / 2, and its log takes
            # V^-1 = I - hat(omega) / 2: the pair is off by |omega x upsilon| / 2 there, by the reference's own formulas
            model = np.linalg.norm(a[3:]) * np.linalg.norm(a[:3]) if float((a[3:] ** 2).sum()) < 1e-20 else 0.0
            assert np.abs(back - a.astype(dt)).max() <= tol * max(1.0, np.abs(a).max()) + model, (a, back)
        rng = np.random.default_rng(43)
        for _ in range(60):
            T = R.load(M.rand_pose(rng, 3.0, 0.8), dt)
            q, t = M.exp(R.log(T), dt)
            assert np.abs(q - T[0]).max() <= tol and np.abs(t - T[1]).max() <= tol * max(1.0, np.abs(T[1]).max())


def test_apply_without_a_stored_pose_is_the_identity():
    rng = np.random.default_rng(5)
    for prev_time in (-1.0, 0.0):
        st = dict(prev_time=prev_time, prevTwc=M.rand_pose(rng), log_relT=rng.normal(0, 1, 6))
        T = M.rand_pose(rng)
        so, out, inv, rs = M.apply(st, T, 3.0)
        assert rs == 0 and out.tobytes() == T.tobytes()
        assert so["prev_time"] == prev_time and np.array_equal(so["prevTwc"], st["prevTwc"]) and np.array_equal(so["log_relT"], st["log_relT"])
        assert np.abs(M.pose_mul(out, inv) - [0, 0, 0, 0, 0, 0, 1]).max() <= 1e-14


def test_apply_resyncs_after_a_jump_and_only_then():
    rng = np.random.default_rng(6)
    prev = M.rand_pose(rng, 2.0)
    st = dict(prev_time=1.0, prevTwc=prev, log_relT=rng.normal(0, 0.2, 6))
    so, out, _, rs = M.apply(st, prev, 1.1)                          # prevTwc == Twc
    assert rs == 0 and np.array_equal(so["prevTwc"], prev)
    for jump in (M.rand_pose(rng, 5.0), M.pose_mul(prev, M.rand_pose(rng, 0.0, 0.01)), prev + np.array([0, 2e-5, 0, 0, 0, 0, 0])):
        so, out2, _, rs = M.apply(st, jump, 1.1)                     # a set_pose-like jump: loop closure, bundle adjustment
        assert rs == 1 and np.array_equal(so["prevTwc"], jump)
        assert so["prev_time"] == 1.0 and np.array_equal(so["log_relT"], st["log_relT"])
    so, _, _, rs = M.apply(st, prev + np.array([0, 5e-6, 0, 0, 0, 0, 0]), 1.1)      # below the threshold
    assert rs == 0 and np.array_equal(so["prevTwc"], prev)
    nan = prev.copy(); nan[0] = np.nan
    assert M.apply(st, nan, 1.1)[3] == 1                             # a NaN coefficient is "not zero"


def test_update_then_apply_reproduces_a_constant_velocity_trajectory():
    T, times, v = M.trajectory()
    st = M.reset_state()
    st = M.update(st, T[0], times[0])                                # the first call only stores
    assert st["prev_time"] == times[0] and np.array_equal(st["prevTwc"], T[0]) and not st["log_relT"].any()
    for k in range(1, len(T) - 1):
        st = M.update(st, T[k], times[k])
        assert np.abs(st["log_relT"] - v).max() <= 1e-10, k
        so, pred, inv, rs = M.apply(st, T[k], times[k + 1])
        assert rs == 0
        assert np.abs(pred - T[k + 1]).max() <= 1e-12 * max(1.0, np.abs(T[k + 1]).max()), k
        assert np.abs(M.pose_mul(pred, inv) - [0, 0, 0, 0, 0, 0, 1]).max() <= 1e-13


def test_condition_of_the_gpu_cases_float64_and_longdouble_agree_on_resynced():
    seen = set()
    for name, st, T, time in M.apply_cases():
        a, b = M.apply(st, T, time), M.apply(st, T, time, np.longdouble)
        assert a[3] == b[3], "float64 and longdouble disagree on resynced (%s): choose another seed" % name
        seen.add(a[3])
        if st["prev_time"] > 0:
            for dt in (np.float64, np.longdouble):
                d = np.abs(M.resync_log(st, T, dt)).astype(np.float64)
                assert (np.abs(d - M.RESYNC_PREC) > 1e-7).all(), "|d_k| within 1e-7 of the threshold (%s): choose another seed" % name
    assert seen == {0, 1}
