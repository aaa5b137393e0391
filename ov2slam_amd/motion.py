"""Host-side mirror of the reference's MotionModel (include/visual_front_end.hpp:38-90) on top of the C ABI (ov2_motion_apply /
ov2_motion_update and their batch forms, csrc/motion.hip):

    apply    applyMotionModel: the resync of prevTwc when the pose was moved, the prediction Twc * exp(log_relT * dt), its inverse
    update   updateMotionModel: log(prevTwc^-1 * Twc) / dt; the first call only stores

A state is a dict named like the fields of ov2_motion_state: prev_time (float), prevTwc (7,), log_relT (6,).  Poses are
[tx ty tz qx qy qz qw], as held by the Frame."""
import ctypes as C

import numpy as np

from . import _lib as L


def reset_state(state=None):
    """MotionModel::reset(): prev_time = -1, log_relT = 0; prevTwc is kept (the identity for a new state)"""
    prev = np.array([0, 0, 0, 0, 0, 0, 1.0]) if state is None else np.array(state["prevTwc"], np.float64).reshape(7)
    return dict(prev_time=-1.0, prevTwc=prev, log_relT=np.zeros(6))


def _states(states):
    S = (L.MotionState * max(1, len(states)))()
    for b, s in enumerate(states):
        S[b].prev_time = float(s["prev_time"])
        S[b].prevTwc[:] = [float(v) for v in np.asarray(s["prevTwc"], np.float64).reshape(7)]
        S[b].log_relT[:] = [float(v) for v in np.asarray(s["log_relT"], np.float64).reshape(6)]
    return S


def _state_dict(s):
    return dict(prev_time=float(s.prev_time), prevTwc=np.array(s.prevTwc[:], np.float64), log_relT=np.array(s.log_relT[:], np.float64))


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def apply_batch(ctx, states, Twc, time):
    """ov2_motion_apply_batch: (states after the resync, Twc_out (n, 7), Tcw_out (n, 7), resynced (n,) uint8)"""
    states = list(states)
    n = len(states)
    T = np.ascontiguousarray(Twc, np.float64).reshape(n, 7)
    tm = np.ascontiguousarray(time, np.float64).reshape(n)
    S, So = _states(states), (L.MotionState * max(1, n))()
    To, Ti, rs = np.zeros((n, 7)), np.zeros((n, 7)), np.zeros(n, np.uint8)
    L.check(ctx.lib.ov2_motion_apply_batch(ctx.h, n, S, _p(T), _p(tm), So, _p(To), _p(Ti), _p(rs)))
    return [_state_dict(So[b]) for b in range(n)], To, Ti, rs


def apply(ctx, state, Twc, time):
    """ov2_motion_apply: (state after the resync, Twc_out (7,), Tcw_out (7,), resynced 0 / 1)"""
    T = np.ascontiguousarray(Twc, np.float64).reshape(7)
    S, So = _states([state]), L.MotionState()
    To, Ti, rs = np.zeros(7), np.zeros(7), np.zeros(1, np.uint8)
    L.check(ctx.lib.ov2_motion_apply(ctx.h, S, _p(T), float(time), C.byref(So), _p(To), _p(Ti), _p(rs)))
    return _state_dict(So), To, Ti, int(rs[0])


def update_batch(ctx, states, Twc, time):
    """ov2_motion_update_batch: the states after updateMotionModel"""
    states = list(states)
    n = len(states)
    T = np.ascontiguousarray(Twc, np.float64).reshape(n, 7)
    tm = np.ascontiguousarray(time, np.float64).reshape(n)
    S, So = _states(states), (L.MotionState * max(1, n))()
    L.check(ctx.lib.ov2_motion_update_batch(ctx.h, n, S, _p(T), _p(tm), So))
    return [_state_dict(So[b]) for b in range(n)]


def update(ctx, state, Twc, time):
    """ov2_motion_update: the state after updateMotionModel"""
    T = np.ascontiguousarray(Twc, np.float64).reshape(7)
    S, So = _states([state]), L.MotionState()
    L.check(ctx.lib.ov2_motion_update(ctx.h, S, _p(T), float(time), C.byref(So)))
    return _state_dict(So)
