"""The device motion model (csrc/motion.hip: ov2_motion_apply / ov2_motion_update and their batch forms) against the numpy
specification (tests/motion_ref.py, checked on the CPU by tests/test_motion_reference.py).

`resynced` is compared EXACTLY with the float64 specification.  CONDITION (asserted in tests/test_motion_reference.py): float64 and
longdouble agree on it on every committed case and no |d_k| lies within 1e-7 of the 1e-5 threshold.

NUMBERS: every double of a case's outputs must lie within

    max(1e-12 max(1, |v|), 100 x max |float64 - longdouble| of the specification's outputs on that case)

-- the rule of tests/test_gpu_posegraph.py: device sin / cos / atan are not libm's, and 100 x is for another order of the same
operations.

EXACT: Tcw_out is ov2_se3_inverse(Twc_out) bit for bit; what a branch copies (the pose when no pose is stored, prevTwc on a resync
or an update, prev_time) is copied bit for bit; the batch call returns the bytes of the single calls; two runs return the same
bytes; a rejected call writes nothing."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import motion_ref as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOOR = 1e-12

_cache = {}


def cases(kind):
    """the committed cases with the specification's answers in float64 and longdouble (computed once per module)"""
    if kind not in _cache:
        out = []
        for name, st, T, time in (M.apply_cases() if kind == "apply" else M.update_cases()):
            f = M.apply if kind == "apply" else M.update
            out.append(dict(name=name, state=st, Twc=T, time=time, want=f(st, T, time), want_ld=f(st, T, time, np.longdouble)))
        _cache[kind] = out
    return _cache[kind]


def _flat_state(s):
    return np.concatenate([[s["prev_time"]], s["prevTwc"], s["log_relT"]]).astype(np.longdouble)


def _flat(kind, res):
    if kind == "apply":
        return np.concatenate([_flat_state(res[0]), np.asarray(res[1], np.longdouble), np.asarray(res[2], np.longdouble)])
    return _flat_state(res)


def _within(kind, c, got):
    want, ld = _flat(kind, c["want"]), _flat(kind, c["want_ld"])
    spread = float(np.abs(want - ld).max())
    tol = np.maximum(FLOOR * np.maximum(1.0, np.abs(want)), 100.0 * spread)
    d = np.abs(_flat(kind, got) - want)
    ratio = float((d / tol).max())
    print("%s %s: float64 - longdouble %.3g, device - spec %.3g, %.3g of its bound" % (kind, c["name"], spread, float(d.max()), ratio))
    assert (d <= tol).all(), (c["name"], d, tol)
    return ratio


def _state_bytes(s):
    return np.concatenate([[s["prev_time"]], s["prevTwc"], s["log_relT"]]).astype(np.float64).tobytes()


@pytest.mark.gpu
def test_apply_against_the_specification(gpu_ctx):
    from ov2slam_amd import keyframe, motion
    worst, n_resynced = 0.0, 0
    for c in cases("apply"):
        got = motion.apply(gpu_ctx, c["state"], c["Twc"], c["time"])
        assert got[3] == c["want"][3], c["name"]
        n_resynced += got[3]
        worst = max(worst, _within("apply", c, got))
        assert got[2].tobytes() == keyframe.se3_inverse(got[1]).tobytes(), c["name"]          # bit for bit
        st = c["state"]
        assert got[0]["prev_time"] == st["prev_time"] and got[0]["log_relT"].tobytes() == np.asarray(st["log_relT"], np.float64).tobytes()
        assert got[0]["prevTwc"].tobytes() == (c["Twc"] if got[3] else st["prevTwc"]).tobytes()
        if not st["prev_time"] > 0:
            assert got[1].tobytes() == c["Twc"].tobytes() and got[3] == 0
    print("worst device - specification difference: %.3g of its bound; %d of %d cases resynced" % (worst, n_resynced, len(cases("apply"))))
    assert 0 < n_resynced < len(cases("apply"))


@pytest.mark.gpu
def test_update_against_the_specification(gpu_ctx):
    from ov2slam_amd import motion
    worst = 0.0
    for c in cases("update"):
        got = motion.update(gpu_ctx, c["state"], c["Twc"], c["time"])
        worst = max(worst, _within("update", c, got))
        assert got["prev_time"] == c["time"] and got["prevTwc"].tobytes() == c["Twc"].tobytes()
        if c["state"]["prev_time"] < 0:                                                       # the first call only stores
            assert got["log_relT"].tobytes() == np.asarray(c["state"]["log_relT"], np.float64).tobytes()
    print("worst device - specification difference: %.3g of its bound" % worst)


@pytest.mark.gpu
def test_a_trajectory_is_predicted(gpu_ctx):
    """apply, then update with the trajectory's pose (as if computePose had found it), frame after frame along a constant-velocity
    trajectory: the model leaves the pose before the second update and predicts the next pose from the third frame on.  Bounds: the
    velocity to 1e-10 (as tests/test_motion_reference.py holds the specification), the prediction to that times the frame interval
    (0.05 s), doubled: 1e-11."""
    from ov2slam_amd import motion
    T, times, v = M.trajectory()
    st, cur = motion.reset_state(), T[0]
    for k in range(len(T)):
        so, pred, inv, rs = motion.apply(gpu_ctx, st, cur, times[k])
        assert rs == 0 and so["prevTwc"].tobytes() == np.asarray(st["prevTwc"], np.float64).tobytes()
        if k == 0:
            assert pred.tobytes() == cur.tobytes()
        else:
            want = cur if k == 1 else T[k]                              # one update: a stored pose, no velocity yet
            assert np.abs(pred - want).max() <= 1e-11 * max(1.0, np.abs(want).max()), k
        st, cur = motion.update(gpu_ctx, so, T[k], times[k]), T[k]
        if k >= 1:
            assert np.abs(st["log_relT"] - v).max() <= 1e-10, k


@pytest.mark.gpu
def test_batch_returns_the_bytes_of_the_single_calls_and_two_runs_agree(gpu_ctx):
    from ov2slam_amd import motion
    ca, cu = cases("apply"), cases("update")
    order = np.random.default_rng(3).permutation(len(ca))
    singles = [motion.apply(gpu_ctx, ca[i]["state"], ca[i]["Twc"], ca[i]["time"]) for i in order]
    args = ([ca[i]["state"] for i in order], np.array([ca[i]["Twc"] for i in order]), np.array([ca[i]["time"] for i in order]))
    a, b = motion.apply_batch(gpu_ctx, *args), motion.apply_batch(gpu_ctx, *args)
    for k, s in enumerate(singles):
        for r in (a, b):
            assert _state_bytes(s[0]) == _state_bytes(r[0][k]) and s[1].tobytes() == r[1][k].tobytes()
            assert s[2].tobytes() == r[2][k].tobytes() and s[3] == r[3][k]
    singles = [motion.update(gpu_ctx, c["state"], c["Twc"], c["time"]) for c in cu]
    args = ([c["state"] for c in cu], np.array([c["Twc"] for c in cu]), np.array([c["time"] for c in cu]))
    a, b = motion.update_batch(gpu_ctx, *args), motion.update_batch(gpu_ctx, *args)
    for k, s in enumerate(singles):
        assert _state_bytes(s) == _state_bytes(a[k]) == _state_bytes(b[k])
    # more items than one work-group (64 lanes) holds, an odd count
    n = 131
    rep = [ca[k % len(ca)] for k in range(n)]
    big = motion.apply_batch(gpu_ctx, [c["state"] for c in rep], np.array([c["Twc"] for c in rep]), np.array([c["time"] for c in rep]))
    for k in range(n):
        s = motion.apply(gpu_ctx, rep[k]["state"], rep[k]["Twc"], rep[k]["time"]) if k >= len(ca) and k % 37 == 0 else None
        j = k % len(ca)
        assert big[1][k].tobytes() == big[1][j].tobytes() and big[2][k].tobytes() == big[2][j].tobytes() and big[3][k] == big[3][j]
        if s is not None:
            assert s[1].tobytes() == big[1][k].tobytes() and _state_bytes(s[0]) == _state_bytes(big[0][k])
    assert motion.apply_batch(gpu_ctx, [], np.zeros((0, 7)), np.zeros(0))[1].shape == (0, 7)
    assert motion.update_batch(gpu_ctx, [], np.zeros((0, 7)), np.zeros(0)) == []


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


@pytest.mark.gpu
def test_rejected_calls_write_nothing(gpu_ctx):
    from ov2slam_amd import _lib as L
    from ov2slam_amd import motion
    lib = gpu_ctx.lib
    n = 3
    cs = cases("apply")[:n]
    good_S = motion._states([c["state"] for c in cs])
    good_T = np.array([c["Twc"] for c in cs])
    good_t = np.array([c["time"] for c in cs])

    def run(S, T, t, null=None, n_items=n):
        """both batch forms with the given inputs; every output pre-filled with a pattern that must survive"""
        So = (L.MotionState * n)()
        C.memset(So, 0x5a, C.sizeof(So))
        To, Ti, rs = np.full((n, 7), 7.25), np.full((n, 7), 7.25), np.full(n, 0x5a, np.uint8)
        before = (bytes(So), To.tobytes(), Ti.tobytes(), rs.tobytes())
        a = [gpu_ctx.h, n_items, S, _p(T), _p(t), So, _p(To), _p(Ti), _p(rs)]
        if null is not None:
            a[null] = None
        assert lib.ov2_motion_apply_batch(*a) == L.OV2_EINVAL
        assert (bytes(So), To.tobytes(), Ti.tobytes(), rs.tobytes()) == before
        if null is None or null <= 5:
            assert lib.ov2_motion_update_batch(*a[:6]) == L.OV2_EINVAL
            assert bytes(So) == before[0]

    for null in (0, 2, 3, 4, 5, 6, 7, 8):                            # NULL context / arrays
        run(good_S, good_T, good_t, null=null)
    run(good_S, good_T, good_t, n_items=-1)
    for bad in (np.nan, np.inf):
        T = good_T.copy(); T[1, 4] = bad
        run(good_S, T, good_t)                                        # a pose that is not finite
        t = good_t.copy(); t[2] = bad
        run(good_S, good_T, t)
        for field, idx in (("prev_time", None), ("prevTwc", 2), ("log_relT", 5)):
            S = motion._states([c["state"] for c in cs])
            if idx is None:
                S[1].prev_time = bad
            else:
                getattr(S[1], field)[idx] = bad
            run(S, good_T, good_t)                                    # a state that is not finite
    for step in (0.0, -0.25):                                         # dt == 0 and dt < 0
        t = good_t.copy(); t[0] = cs[0]["state"]["prev_time"] + step
        run(good_S, good_T, t)
    S = motion._states([dict(c["state"], prev_time=0.0) for c in cs])
    run(S, good_T, np.zeros(n))                                       # prev_time == 0 counts as a stored time
    # the single forms
    s1, T1 = motion._states([cs[0]["state"]]), good_T[0].copy()
    So = L.MotionState(); C.memset(C.byref(So), 0x5a, C.sizeof(So)); keep = bytes(So)
    To, Ti, rs = np.full(7, 7.25), np.full(7, 7.25), np.full(1, 0x5a, np.uint8)
    assert lib.ov2_motion_apply(gpu_ctx.h, s1, _p(T1), float(cs[0]["state"]["prev_time"]), C.byref(So), _p(To), _p(Ti), _p(rs)) == L.OV2_EINVAL
    assert lib.ov2_motion_update(gpu_ctx.h, s1, _p(T1), float(cs[0]["state"]["prev_time"]), C.byref(So)) == L.OV2_EINVAL
    assert lib.ov2_motion_apply(gpu_ctx.h, s1, None, 100.0, C.byref(So), _p(To), _p(Ti), _p(rs)) == L.OV2_EINVAL
    assert lib.ov2_motion_update(gpu_ctx.h, None, _p(T1), 100.0, C.byref(So)) == L.OV2_EINVAL
    assert bytes(So) == keep and (To == 7.25).all() and (Ti == 7.25).all() and rs[0] == 0x5a
    with pytest.raises(L.Ov2Error):
        motion.update(gpu_ctx, cs[0]["state"], good_T[0], cs[0]["state"]["prev_time"])


def _wr(f, a):
    a = np.ascontiguousarray(a)
    f.write(np.int64(a.nbytes).tobytes()); f.write(a.tobytes())


def _rd(f, dt):
    nb = int(np.frombuffer(f.read(8), np.int64)[0])
    return np.frombuffer(f.read(nb), dt)


@pytest.mark.gpu
def test_cpp_adapter(gpu_ctx, tmp_path):
    """tests/cpp/motion_run.cpp: ov2::MotionModel played over a trajectory with one moved pose returns the bytes of the Python path"""
    from ov2slam_amd import motion
    exe = tmp_path / "motion_run"
    libdir = os.path.join(ROOT, "ov2slam_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "motion_run.cpp"),
                           "-o", str(exe), "-L", libdir, "-lov2slam_hip", "-Wl,-rpath," + libdir])
    T, times, _ = M.trajectory()
    A = np.concatenate([T[:1], T[:-1]])                       # the pose a frame starts with: the one the last frame ended with
    A[4] = M.pose_mul(A[4], M.rand_pose(np.random.default_rng(2), 0.3, 0.1))       # moved between two frames: resynced
    cf, rf = tmp_path / "case.bin", tmp_path / "res.bin"
    with open(cf, "wb") as f:
        _wr(f, A); _wr(f, T); _wr(f, times)
    r = subprocess.run([str(exe), str(cf), str(rf)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    with open(rf, "rb") as f:
        pred, inv, rs, states, refused = _rd(f, np.float64), _rd(f, np.float64), _rd(f, np.uint8), _rd(f, np.float64), _rd(f, np.int32)
    st = motion.reset_state()
    for k in range(len(T)):
        st, p, i, r1 = motion.apply(gpu_ctx, st, A[k], times[k])
        assert p.tobytes() == pred[7 * k:7 * k + 7].tobytes() and i.tobytes() == inv[7 * k:7 * k + 7].tobytes() and r1 == rs[k]
        st = motion.update(gpu_ctx, st, T[k], times[k])
        assert _state_bytes(st) == states[14 * k:14 * k + 14].tobytes()
    assert list(rs) == [0, 0, 0, 0, 1, 0] and refused[0] == 1
