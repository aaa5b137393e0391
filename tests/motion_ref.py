"""The specification of the device motion model (ov2_motion_apply / ov2_motion_update, ov2slam_amd/csrc/motion.hip) in numpy, generic
over the dtype (float64, numpy.longdouble): MotionModel::applyMotionModel and updateMotionModel of the reference's
include/visual_front_end.hpp:38-90 on Sophus' SE(3) product, inverse and log as tests/posegraph_ref.py writes them (pinned to the
reference's compiled code by tests/test_posegraph_reference.py), and SE3::exp as the body of that file's `plus` without the product.

A state is a dict prev_time, prevTwc (7,), log_relT (6,); poses are [t q].  One item per call: the model is a handful of scalars."""
import numpy as np

from tests import posegraph_ref as R

RESYNC_PREC = 1e-5                 # isZero(1.e-5), :48


def exp(a, dt=np.float64):
    """Sophus SE3::exp of (n, 6) [upsilon; omega] -> (q, t) (se3.hpp:763-784, so3.hpp:585-621)"""
    a = np.asarray(a, dt).reshape(-1, 6)
    d = a.dtype.type
    om = a[:, 3:]
    tsq = (om * om).sum(1)
    small = tsq < d(R.EPS) * d(R.EPS)
    theta = np.where(small, d(0), np.sqrt(tsq))
    th = np.where(small, d(1), theta)
    t4 = tsq * tsq
    imag = np.where(small, d(0.5) - tsq / d(48) + t4 / d(3840), np.sin(d(0.5) * th) / th)
    real = np.where(small, d(1) - tsq / d(8) + t4 / d(384), np.cos(d(0.5) * th))
    qe = np.concatenate([imag[:, None] * om, real[:, None]], axis=1)
    O = R.hat(om)
    tq = np.where(small, d(1), tsq)
    V = np.eye(3, dtype=a.dtype)[None] + ((d(1) - np.cos(th)) / tq)[:, None, None] * O + ((th - np.sin(th)) / (tq * th))[:, None, None] * (O @ O)
    V = np.where((theta < d(R.EPS))[:, None, None], R.quat_to_R(qe), V)
    return qe, np.einsum("nij,nj->ni", V, a[:, :3])


def reset_state(prevTwc=(0, 0, 0, 0, 0, 0, 1.0)):
    return dict(prev_time=-1.0, prevTwc=np.array(prevTwc, np.float64), log_relT=np.zeros(6))


def _state(s, dt):
    return dict(prev_time=dt(s["prev_time"]), prevTwc=np.asarray(s["prevTwc"], dt).reshape(7).copy(),
                log_relT=np.asarray(s["log_relT"], dt).reshape(6).copy())


def se3_inverse(T, dt=np.float64):
    """ov2_se3_inverse: the conjugate, the rotation matrix of the conjugate written out, each sum of three terms serial"""
    T = np.asarray(T, dt).reshape(7)
    d = T.dtype.type
    x, y, z, w = -T[3], -T[4], -T[5], T[6]
    Rm = np.array([[d(1) - d(2) * (y * y + z * z), d(2) * (x * y - z * w), d(2) * (x * z + y * w)],
                   [d(2) * (x * y + z * w), d(1) - d(2) * (x * x + z * z), d(2) * (y * z - x * w)],
                   [d(2) * (x * z - y * w), d(2) * (y * z + x * w), d(1) - d(2) * (x * x + y * y)]], dt)
    t = np.array([-((Rm[r, 0] * T[0] + Rm[r, 1] * T[1]) + Rm[r, 2] * T[2]) for r in range(3)], dt)
    return np.concatenate([t, [x, y, z, w]]).astype(dt)


def resync_log(state, Twc, dt=np.float64):
    """d = (Twc * prevTwc^-1).log(), the six numbers isZero(1.e-5) looks at"""
    s = _state(state, dt)
    return R.log(R.mul(R.load(Twc, dt), R.inv(R.load(s["prevTwc"], dt))))[0]


def apply(state, Twc, time, dt=np.float64):
    """applyMotionModel -> (state_out, Twc_out (7,), Tcw_out (7,), resynced)"""
    s = _state(state, dt)
    Twc = np.asarray(Twc, dt).reshape(7)
    time = dt(time)
    resynced = 0
    if s["prev_time"] > 0:
        d = resync_log(state, Twc, dt)
        if not bool((np.abs(d) <= dt(RESYNC_PREC)).all()):          # a NaN is "not zero"
            s["prevTwc"] = Twc.copy()
            resynced = 1
        v = s["log_relT"] * (time - s["prev_time"])
        out = R.store(R.mul(R.load(Twc, dt), exp(v, dt)))[0]
    else:
        out = Twc.copy()
    return s, out, se3_inverse(out, dt), resynced


def update(state, Twc, time, dt=np.float64):
    """updateMotionModel -> state_out"""
    s = _state(state, dt)
    Twc = np.asarray(Twc, dt).reshape(7)
    time = dt(time)
    if not s["prev_time"] < 0:
        step = time - s["prev_time"]
        s["log_relT"] = R.log(R.mul(R.inv(R.load(s["prevTwc"], dt)), R.load(Twc, dt)))[0] / step
    s["prev_time"] = time
    s["prevTwc"] = Twc.copy()
    return s


# ----------------------------------------------------------------------------------------------------------- the committed cases
def rand_pose(rng, t_scale=1.0, rot=0.4):
    w = rng.normal(0, rot, 3)
    th = np.linalg.norm(w)
    return np.concatenate([rng.normal(0, t_scale, 3), np.sin(th / 2) * w / th, [np.cos(th / 2)]])


def pose_mul(A, B, dt=np.float64):
    return R.store(R.mul(R.load(A, dt), R.load(B, dt)))[0]


def apply_cases(seed=19):
    """(name, state, Twc, time): what tests/test_gpu_motion.py runs through ov2_motion_apply.  Every branch: no pose stored
    (prev_time -1 and 0), the pose where the update left it (no resync), moved by a rotation / a translation / both (resync),
    moved by less than the threshold (1e-7: no resync), zero velocity, a velocity whose rotation over dt is below Sophus'
    small-angle switch, a long dt (a rotation of several radians)."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(24):
        prev = rand_pose(rng, 3.0)
        vel = np.concatenate([rng.normal(0, 0.5, 3), rng.normal(0, 0.3, 3)])
        st = dict(prev_time=1.0 + k, prevTwc=prev, log_relT=vel)
        step = (0.05, 0.1, 0.5)[k % 3]
        kind = k % 8
        Twc, name = prev.copy(), "same"
        if kind == 1:
            Twc, name = pose_mul(prev, rand_pose(rng, 0.0, 0.05)), "rotated"
        elif kind == 2:
            Twc, name = prev + np.concatenate([rng.normal(0, 0.2, 3), np.zeros(4)]), "translated"
        elif kind == 3:
            Twc, name = rand_pose(rng, 3.0), "elsewhere"
        elif kind == 4:
            Twc, name = pose_mul(prev, rand_pose(rng, 1e-7, 1e-7)), "moved_below_threshold"
        elif kind == 5:
            st["log_relT"], name = np.zeros(6), "zero_velocity"
        elif kind == 6:
            st["log_relT"], name = np.concatenate([vel[:3], rng.normal(0, 1e-11, 3)]), "small_angle"
        elif kind == 7:
            step, name = 20.0, "long_dt"
        out.append(("%s_%d" % (name, k), st, Twc, st["prev_time"] + step))
    out.append(("reset", reset_state(rand_pose(rng)), rand_pose(rng), 0.5))
    out.append(("prev_time_zero", dict(prev_time=0.0, prevTwc=rand_pose(rng), log_relT=rng.normal(0, 0.1, 6)), rand_pose(rng), 0.5))
    return out


def update_cases(seed=23):
    """(name, state, Twc, time) for ov2_motion_update: the first call (stores), prev_time 0, generic steps, a step that is a
    rotation below the small-angle switch, no motion at all, a rotation close to pi"""
    rng = np.random.default_rng(seed)
    out = [("first", reset_state(rand_pose(rng)), rand_pose(rng), 0.25),
           ("prev_time_zero", dict(prev_time=0.0, prevTwc=rand_pose(rng), log_relT=np.zeros(6)), rand_pose(rng), 0.5)]
    for k in range(16):
        prev = rand_pose(rng, 3.0)
        st = dict(prev_time=2.0 + k, prevTwc=prev, log_relT=rng.normal(0, 0.2, 6))
        kind = k % 4
        if kind == 0:
            Twc, name = pose_mul(prev, rand_pose(rng, 0.1, 0.05)), "step"
        elif kind == 1:
            Twc, name = pose_mul(prev, rand_pose(rng, 1e-3, 1e-11)), "small_angle"
        elif kind == 2:
            Twc, name = prev.copy(), "still"
        else:
            ax = rng.normal(0, 1, 3); ax /= np.linalg.norm(ax)
            ang = np.pi - 10.0 ** rng.uniform(-6, -1)
            Twc, name = pose_mul(prev, np.concatenate([rng.normal(0, 1, 3), np.sin(ang / 2) * ax, [np.cos(ang / 2)]])), "near_pi"
        out.append(("%s_%d" % (name, k), st, Twc, st["prev_time"] + (0.05, 0.1, 1.0)[k % 3]))
    return out


def trajectory(n=6, seed=31, step=0.05):
    """a constant-velocity trajectory: T_k = T_0 exp(v step)^k, times t_0 + k step"""
    rng = np.random.default_rng(seed)
    v = np.concatenate([rng.normal(0, 1.0, 3), rng.normal(0, 0.5, 3)])
    T = [rand_pose(rng, 2.0)]
    E = R.store(exp(v * step))[0]
    for _ in range(n - 1):
        T.append(pose_mul(T[-1], E))
    return np.array(T), 1.0 + step * np.arange(n), v
