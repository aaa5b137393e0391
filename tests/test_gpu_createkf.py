"""ov2_btracker_create_keyframe (csrc/trackb_keyframe.hip, csrc/createkf.hip: MapManager::createKeyframe for the flagged items of a lock-step
batch in one enqueue) against the route of separate calls it replaces (tests/createkf_ref.py: route).  Tracker A plays the rounds of
tests/createkf_cases.py through route(), tracker B through the fused call, on the same frames; EVERY comparison is on raw bytes: both
sides run the same device code on the same inputs, so equality is the requirement, not a tolerance.  Compared per round: the records,
px, lmid, unpx, bv, desc, valid, colour (the whole arrays, which start from the same poison on both sides: an untouched slot stays
poison) and the adaptive state.

Residency: between the rounds both trackers play trackMono steps (doepipolar 1) on the keypoints of the keyframes installed last --
on side A by setKeyframe + setKeyframeInfo, on side B by the device -- and every field of every record, the resident pose and the
motion state are byte-equal.  Before each such step one item's pose is set wrong, so that the 33 % rule fires there and _end's host
re-run reads the keyframe mirror the fused call left on the host.

What the rounds are for is asserted on the CPU in tests/test_createkf_cases.py; here only that the route reaches the actions."""
import ctypes as C

import numpy as np
import pytest

import ov2slam_amd
from ov2slam_amd import _lib as L
from ov2slam_amd import pose
from tests import camera_cases as CAM
from tests import createkf_cases as CC
from tests import createkf_ref as CR
from tests import resident_ref as RR
from tests.match_ref import _inv_act
from tests.test_gpu_frameepi import _epi_params
from tests.test_gpu_framepose import _invert, _params
from tests.test_gpu_priors_lockstep import DIST, K, _wrong
from tests.test_gpu_trackmono import DT, _same_mono_step, _truth

pytestmark = pytest.mark.gpu

W, H, BATCH, N_MAX = CC.W, CC.H, CC.BATCH, CC.N_MAX
POISON = 0x5A
_RUNS = {}


def _tracker(ctx, cal, n_max=N_MAX):
    t = ov2slam_amd.LockstepTracker(ctx, BATCH, W, H, use_clahe=False, nbmaxkps=n_max)
    if cal is not None:
        t.setCalibration(cal)
    return t


def _cal(ctx):
    return ov2slam_amd.CameraCalibration(ctx, "pinhole", *K, D=DIST)


def _state0(detector):
    return np.full(BATCH, CC.FAST_TH0, np.int32) if detector == "gridfast" else np.full(BATCH, CC.QUALITY0, np.float64)


def _poison():
    o = CR.empty_out(BATCH, N_MAX)
    for a in o.values():
        a.view(np.uint8)[...] = POISON
    return o


def _imgs(f, na=BATCH):
    return [CC.frames()[b][0][f] for b in range(na)]


def _mono_args(cal, f, kf):
    """a trackMono step on frame f: the keypoints of the keyframes installed last (kf[b] = (px, lmid) or None), map points that project
    onto the true track under the true pose"""
    rng = np.random.default_rng(700 + f)
    Kc = tuple(float(v) for v in cal.K)
    kps = np.zeros((BATCH, N_MAX, 2), np.float32); wpt = np.zeros((BATCH, N_MAX, 3)); is3d = np.zeros((BATCH, N_MAX), np.uint8)
    lmid = np.zeros((BATCH, N_MAX), np.int32); n = np.zeros(BATCH, np.int32)
    for b in range(BATCH):
        if kf[b] is None or f == 0:
            continue
        px, ids = kf[b]
        m = len(px)
        if not m:
            continue
        gt = (CC.flow(b, px, f - 1, f) + rng.normal(0, 0.3, (m, 2))).astype(np.float32)
        T = _invert(_truth(b)[f])
        bv = cal.computeKeypoints(gt)[1]
        Pc = bv / bv[:, 2:3] * rng.uniform(2, 10, (m, 1))
        for i in range(m):
            wpt[b, i] = _inv_act(T, Pc[i])
        kps[b, :m], lmid[b, :m], n[b] = px, ids, m
        is3d[b, :m] = rng.uniform(size=m) < 0.7
    fkf = dict(_epi_params(True, False, Kc=Kc)["fkf"], nbmaxkps=CC.BASE["nbmaxkps"])
    seeds = lambda: rng.integers(0, 1 << 63, BATCH).astype(np.uint64) * np.uint64(2) + np.uint64(1)
    return ((_imgs(f), kps, wpt, is3d, n, _params(pose.LMEDS, False, Kc), dict(_epi_params(True, False, Kc=Kc), fkf=fkf), np.zeros(BATCH, np.uint8), seeds(),
             lmid, np.full(BATCH, 3, np.int32), seeds(), np.full(BATCH, 10.0 + f * DT + 0.02), np.array([100 * b + f for b in range(BATCH)], np.int32)),
            dict(localba_is_on=np.zeros(BATCH, np.uint8), dop3p=False, n_rows=40))


def _mono_step(t, a, kw):
    out, st, rule, epis, poses, monos = t.trackMono(*a, **kw)
    n = a[4]
    return dict(out=out, st=st, rule=rule, epis=epis, poses=poses, monos=monos, res_T=np.array([t.getPose(b) for b in range(BATCH)]),
                res_s=[t.getMotion(b) for b in range(BATCH)], kp=[t.lastKeypoints(b, int(n[b])) for b in range(BATCH)],
                pr=[t.lastPriors(b, int(n[b])) for b in range(BATCH)], inputs=[t.lastPoseInputs(b) for b in range(BATCH)],
                einputs=[t.lastEpiInputs(b) for b in range(BATCH)])


def _round(ctx, t, cal, ri, detector, how, state):
    r, x = CC.ROUNDS[ri], CC.round_inputs(ri)
    p = CC.round_params(r, detector)
    Twc = x["Twc"] if r["twc"] == "given" else None
    a = (r["n_active"], x["px"], x["lmid"], x["is3d"], x["n"], x["make_kf"], x["nlmid"], x["nkfid"], x["time"], p, state)
    if how == "route":
        return CR.route(ctx, t, cal, *a, Twc=Twc, out=_poison())
    if how == "fused":
        return t.createKeyframe(*a, Twc=Twc, out=_poison())
    t.createKeyframeBegin(*a, Twc=Twc)
    return t.createKeyframeEnd(out=_poison())


def _play(ctx, detector, how, camera=None):
    """frame 0 and its round, a trackMono step on frame 1, the rounds of frame 1, a trackMono step on frame 2 -- on a fresh tracker,
    through 'route', 'fused' (the one-call form) or 'halves', under the EuRoC calibration or a camera of tests/camera_cases.py.
    Computed once and shared; nobody changes a result."""
    key = (detector, how) if camera is None else (detector, how, camera)
    if key in _RUNS:
        return _RUNS[key]
    cal = CAM.calibration(ctx, camera) if camera else _cal(ctx)
    t = _tracker(ctx, cal)
    state = _state0(detector)
    for b in range(BATCH):
        t.setPose(b, _truth(b)[0])
    kf = [None] * BATCH
    rounds, steps = [], []
    for f in range(CC.NFRAMES):
        if f > 0:
            t.setPose(f, _invert(_wrong(_invert(_truth(f)[f]), np.random.default_rng(40 + f), float(cal.K[0]))))      # item f: the rule fires
        a, kw = _mono_args(cal, f, kf)
        steps.append(_mono_step(t, a, kw))
        for b in range(BATCH):                                         # the estimator puts the frames where they belong
            t.setPose(b, _truth(b)[f])
        for ri, r in enumerate(CC.ROUNDS):
            if r["frame"] != f:
                continue
            recs, out = _round(ctx, t, cal, ri, detector, how, state)
            rounds.append(dict(name=r["name"], recs=recs, out=out, state=state.copy()))
            for b, rec in enumerate(recs):
                if rec["action"] == L.OV2_CKF_CREATED:
                    kf[b] = (out["px"][b, :rec["n_kf"]].copy(), out["lmid"][b, :rec["n_kf"]].copy())
    t.close()
    _RUNS[key] = dict(rounds=rounds, steps=steps)
    return _RUNS[key]


def _same_round(a, b, where):
    assert a["recs"] == b["recs"], (where, a["recs"], b["recs"])
    for k in a["out"]:
        assert a["out"][k].tobytes() == b["out"][k].tobytes(), (where, k)
    assert a["state"].tobytes() == b["state"].tobytes(), (where, "adaptive state", a["state"], b["state"])


def _same_play(A, B, where):
    for a, b in zip(A["rounds"], B["rounds"]):
        _same_round(a, b, (where, a["name"]))
    for f, (a, b) in enumerate(zip(A["steps"], B["steps"])):
        _same_mono_step(a, b, (where, "trackMono", f))


def _show(name, A):
    for r in A["rounds"]:
        print(name, r["name"], [(x["action"], x["n_prev"], x["noccupcells"], x["nb2detect"], x["n_new"], x["n_kf"], x["nb3dkps"]) for x in r["recs"]],
              r["state"].tolist())
    for f, s in enumerate(A["steps"]):
        print(name, "step", f, "rule", s["rule"].astype(int).tolist(), [(m["kf"]["n"], m["kf"]["decision"], m["kf"]["reason"]) for m in s["monos"]])


@pytest.mark.parametrize("detector", ["singlescale", "gridfast"])
def test_fused_call_equals_the_route(gpu_ctx, detector):
    A, B = _play(gpu_ctx, detector, "route"), _play(gpu_ctx, detector, "fused")
    _show(detector, A)
    _same_play(A, B, detector)


@pytest.mark.parametrize("camera", CAM.ADDED)
def test_fused_call_equals_the_route_under_added_cameras(gpu_ctx, oracle, camera):
    """The single-scale play under the added cameras of tests/camera_cases.py: fused against route byte for byte, and every created
    keyframe's unpx / bv equal ov2_compute_keypoints on its px as bits and the oracle within the camera's bound; the same for
    lastKeypoints after the trackMono steps in between."""
    cal = CAM.calibration(gpu_ctx, camera)
    A, B = _play(gpu_ctx, "singlescale", "route", camera), _play(gpu_ctx, "singlescale", "fused", camera)
    _show(camera, A)
    _same_play(A, B, camera)
    created = 0
    for r in B["rounds"]:
        for b, rec in enumerate(r["recs"]):
            if rec["action"] != L.OV2_CKF_CREATED or not rec["n_kf"]:
                continue
            m = rec["n_kf"]
            px = np.ascontiguousarray(r["out"]["px"][b, :m])
            su, sb = cal.computeKeypoints(px)
            assert np.array_equal(r["out"]["unpx"][b, :m].view(np.uint32), su.view(np.uint32)), (r["name"], b)
            assert np.array_equal(r["out"]["bv"][b, :m].view(np.uint64), sb.view(np.uint64)), (r["name"], b)
            CAM.assert_keypoints_match_oracle(oracle, camera, px, su, sb)
            created += 1
    assert created >= 8
    for f, s in enumerate(B["steps"]):
        n = np.array([len(k[0]) for k in s["kp"]])
        CAM.assert_step_anchor(gpu_ctx, oracle, cal, camera, dict(n=n), s)
    for f in (1, 2):
        assert A["steps"][f]["rule"][f], (f, A["steps"][f]["rule"])


@pytest.mark.parametrize("detector", ["singlescale", "gridfast"])
def test_the_route_reaches_the_actions(gpu_ctx, detector):
    """on the route's side alone (what the scenes are is asserted without a GPU in tests/test_createkf_cases.py)"""
    A = _play(gpu_ctx, detector, "route")
    by = {r["name"]: r for r in A["rounds"]}
    act = lambda name: [x["action"] for x in by[name]["recs"]]
    assert act("first") == [L.OV2_CKF_CREATED] * 4 and all(x["n_prev"] == 0 and x["n_new"] > 0 for x in by["first"]["recs"])
    assert act("mixed") == [L.OV2_CKF_CREATED, L.OV2_CKF_CREATED, L.OV2_CKF_NOT_REQUESTED, L.OV2_CKF_OVERFLOW]
    assert by["mixed"]["recs"][1]["nb2detect"] <= 0 and by["mixed"]["recs"][1]["n_new"] == 0
    assert act("short") == [L.OV2_CKF_DUP_LMID, L.OV2_CKF_NOT_REQUESTED, L.OV2_CKF_CREATED] and by["short"]["recs"][0]["n_new"] > 0
    assert [x["n_kf"] for x in by["sizes"]["recs"]] == [1, 2, 64, 65] and [x["n_kf"] for x in by["full"]["recs"]] == [160, 128, 129, 0]
    assert act("sizes") == act("full") == [L.OV2_CKF_CREATED] * 4
    # the adaptive state: moved by the rounds that detect, also where the item overflowed or repeated an id; untouched elsewhere
    s0 = _state0(detector)
    assert by["first"]["state"].tobytes() != s0.tobytes()
    assert by["mixed"]["state"][1] == by["first"]["state"][1] and by["mixed"]["state"][2] == by["first"]["state"][2]
    assert by["sizes"]["state"].tobytes() == by["short"]["state"].tobytes() == by["full"]["state"].tobytes()
    # output slots: nothing of an unflagged, overflowing or repeating item is written; invalid descriptors exist; no BRIEF without use_brief
    po = _poison()
    for name, b in (("mixed", 2), ("mixed", 3), ("short", 0), ("short", 1), ("short", 3)):
        for k, a in by[name]["out"].items():
            assert a[b].tobytes() == po[k][b].tobytes(), (name, b, k)
    m = by["mixed"]["recs"][0]
    v = by["mixed"]["out"]["valid"][0, :m["n_kf"]]
    assert set(v.tolist()) == {0, 1} and not by["mixed"]["out"]["desc"][0, :m["n_kf"]][v == 0].any()
    assert by["sizes"]["out"]["desc"].tobytes() == po["desc"].tobytes() and by["sizes"]["out"]["valid"].tobytes() == po["valid"].tobytes()
    c = by["mixed"]["out"]["color"][0]
    assert (c[:m["n_prev"]] == POISON).all() and len(set(c[m["n_prev"]:m["n_kf"]].tolist())) > 3
    # the residency steps: the rule fired on the item whose pose was set wrong, and keypoints of the installed keyframes were tracked
    for f in (1, 2):
        s = A["steps"][f]
        assert s["rule"][f], (f, s["rule"])
        assert sum(int(((s["st"][b] & 3) == 1).sum()) for b in range(BATCH)) >= 40, f
        assert any(mo["kf"]["n"] > 0 for mo in s["monos"]), f                 # the join by lmid found the keyframe's ids


def test_begin_end_equals_the_one_call_form(gpu_ctx):
    _same_play(_play(gpu_ctx, "singlescale", "fused"), _play(gpu_ctx, "singlescale", "halves"), "halves")


def test_a_second_run_on_fresh_trackers_gives_the_same_bytes(gpu_ctx):
    first = _play(gpu_ctx, "gridfast", "fused")
    del _RUNS[("gridfast", "fused")]
    try:
        again = _play(gpu_ctx, "gridfast", "fused")
    finally:
        _RUNS[("gridfast", "fused")] = first
    _same_play(first, again, "repeat")


def test_rejected_calls_leave_the_tracker_usable(gpu_ctx):
    """every refusal comes before anything is enqueued: the outputs, the adaptive state and the tracker stay as they were, and the round
    played afterwards equals the one a fresh tracker plays"""
    ctx, cal = gpu_ctx, _cal(gpu_ctx)
    ref = _play(ctx, "singlescale", "fused")
    x, p = CC.round_inputs(0), CC.round_params(CC.ROUNDS[0], "singlescale")
    base = dict(n_active=4, px=x["px"], lmid=x["lmid"], is3d=x["is3d"], n=x["n"], make_kf=x["make_kf"], nlmid=x["nlmid"], nkfid=x["nkfid"],
                time=x["time"], params=p, Twc=x["Twc"])

    def refused(t, code, words, **change):
        a = dict(base, **change)
        det = "gridfast" if a["params"]["detector"] == "gridfast" else "singlescale"
        state, out = _state0(det), _poison()
        with pytest.raises(ov2slam_amd.Ov2Error) as err:
            t.createKeyframe(a["n_active"], a["px"], a["lmid"], a["is3d"], a["n"], a["make_kf"], a["nlmid"], a["nkfid"], a["time"], a["params"],
                             state, Twc=a["Twc"], out=out)
        assert err.value.code == code and words in str(err.value), (words, str(err.value))
        assert state.tobytes() == _state0(det).tobytes() and all(out[k].tobytes() == v.tobytes() for k, v in _poison().items())

    fresh = _tracker(ctx, cal)
    refused(fresh, L.OV2_EINVAL, "no current frames")
    z2, z3, z1 = np.zeros((BATCH, N_MAX, 2), np.float32), np.zeros((BATCH, N_MAX, 3)), np.zeros((BATCH, N_MAX), np.uint8)
    fresh.trackFrame(_imgs(0), z2, z2, None, np.zeros(BATCH, np.int32))
    refused(fresh, L.OV2_EINVAL, "resident pose", Twc=None)
    fresh.close()
    nocal = _tracker(ctx, None)
    nocal.trackFrame(_imgs(0), z2, z2, None, np.zeros(BATCH, np.int32))
    refused(nocal, L.OV2_EINVAL, "calibration")
    nocal.close()

    t = _tracker(ctx, cal)
    for b in range(BATCH):
        t.setPose(b, _truth(b)[0])
    a0, kw0 = _mono_args(cal, 0, [None] * BATCH)
    t.trackMono(*a0, **kw0)
    for b in range(BATCH):
        t.setPose(b, _truth(b)[0])
    refused(t, L.OV2_EINVAL, "n_active", n_active=0)
    c = t._marshal_create_keyframe(4, x["px"], x["lmid"], x["is3d"], x["n"], x["make_kf"], x["nlmid"], x["nkfid"], x["time"], p,
                                   _state0("singlescale"), x["Twc"])
    assert t.lib.ov2_btracker_create_keyframe_begin(t.h_trk, BATCH + 1, *c.args[1:]) == L.OV2_EINVAL
    assert b"n_active" in t.lib.ov2_last_error() and c.keep["state"].tobytes() == _state0("singlescale").tobytes()
    for bad in (-1, N_MAX + 1):
        n = x["n"].copy(); n[1] = bad
        refused(t, L.OV2_EINVAL, "cfg.n_max slots", n=n)
    refused(t, L.OV2_EINVAL, "ncellsize", params=dict(p, ncellsize=0))
    refused(t, L.OV2_EINVAL, "at least 8", params=dict(p, det_cell=4))
    refused(t, L.OV2_EUNSUPPORTED, "[8,64]", params=dict(p, det_cell=100))
    refused(t, L.OV2_EINVAL, "detectGFTT", params=dict(p, detector="gftt"))
    refused(t, L.OV2_EINVAL, "mask_mode", params=dict(p, detector="gridfast", mask_mode=7))
    n1 = x["n"].copy(); n1[2] = 2
    for bad in (-1, int(x["nlmid"][2])):
        lm = x["lmid"].copy(); lm[2, 0], lm[2, 1] = 0, bad
        refused(t, L.OV2_EINVAL, "monotone", n=n1, lmid=lm)
    nl = x["nlmid"].copy(); nl[0] = 2 ** 31 - 1 - 100
    refused(t, L.OV2_EINVAL, "overflows int", nlmid=nl)
    tm = x["time"].copy(); tm[3] = np.inf
    refused(t, L.OV2_EINVAL, "time not finite", time=tm)
    Tw = x["Twc"].copy(); Tw[1, 2] = np.nan
    refused(t, L.OV2_EINVAL, "pose not finite", Twc=Tw)
    # through the C ABI: NULL params / input / arrays, a NULL state array
    cp, ci = L.CreateKeyframeParams(), L.CreateKeyframeInput()
    assert t.lib.ov2_btracker_create_keyframe_begin(t.h_trk, 4, None, C.byref(ci)) == L.OV2_EINVAL
    assert t.lib.ov2_btracker_create_keyframe_begin(t.h_trk, 4, C.byref(cp), None) == L.OV2_EINVAL
    assert t.lib.ov2_btracker_create_keyframe_begin(t.h_trk, 4, C.byref(cp), C.byref(ci)) == L.OV2_EINVAL and b"NULL px_h" in t.lib.ov2_last_error()
    assert t.lib.ov2_btracker_create_keyframe_end(t.h_trk, None, None, None, None, None, None, None, None) == L.OV2_EINVAL
    # what is NOT refused: a bad id on an item that is not flagged
    lm = x["lmid"].copy(); lm[2, 1] = -5
    mk = x["make_kf"].copy(); mk[2] = 0
    state = _state0("singlescale")
    recs, _ = t.createKeyframe(4, x["px"], lm, x["is3d"], n1, mk, x["nlmid"], x["nkfid"], x["time"], p, state, Twc=x["Twc"])
    assert [r["action"] for r in recs] == [L.OV2_CKF_CREATED, L.OV2_CKF_CREATED, L.OV2_CKF_NOT_REQUESTED, L.OV2_CKF_CREATED]
    # the tracker is where it was: the round a fresh tracker plays, with the same bytes
    state = _state0("singlescale")
    recs, out = _round(ctx, t, cal, 0, "singlescale", "fused", state)
    _same_round(dict(recs=recs, out=out, state=state), ref["rounds"][0], "after the refusals")
    # an open call refuses the calls that would change what it works on, and a step; an open step refuses the call
    a = (4, x["px"], x["lmid"], x["is3d"], x["n"], x["make_kf"], x["nlmid"], x["nkfid"], x["time"], p, state)
    t.createKeyframeBegin(*a, Twc=x["Twc"])
    for call in (lambda: t.createKeyframeBegin(*a, Twc=x["Twc"]), lambda: t.setPose(0, _truth(0)[0]), lambda: t.setKeyframeInfo(0, 1, 2.0, 3),
                 lambda: t.setKeyframe(0, np.zeros(0, np.int32), np.zeros((0, 2), np.float32), np.zeros((0, 3)), _truth(0)[0]),
                 lambda: t.trackFrameBegin(_imgs(1), z2, z2, None, np.zeros(BATCH, np.int32))):
        with pytest.raises(ov2slam_amd.Ov2Error) as err:
            call()
        assert err.value.code == L.OV2_EINVAL
    t.createKeyframeEnd()
    with pytest.raises(ov2slam_amd.Ov2Error):
        t.createKeyframeEnd()
    t.trackFrameBegin(_imgs(1), z2, z2, None, np.zeros(BATCH, np.int32))
    refused(t, L.OV2_EINVAL, "a step is open")
    t.trackFrameEnd()
    t.close()
    big = _tracker(ctx, cal, n_max=L.OV2_FKF_MAX_POINTS + 1)
    big.trackFrame(_imgs(0), np.zeros((BATCH, big.n_max, 2), np.float32), np.zeros((BATCH, big.n_max, 2), np.float32), None, np.zeros(BATCH, np.int32))
    with pytest.raises(ov2slam_amd.Ov2Error) as err:
        big.createKeyframe(4, np.zeros((BATCH, big.n_max, 2), np.float32), np.zeros((BATCH, big.n_max), np.int32), np.zeros((BATCH, big.n_max), np.uint8),
                           x["n"], x["make_kf"], x["nlmid"], x["nkfid"], x["time"], p, _state0("singlescale"), Twc=x["Twc"])
    assert err.value.code == L.OV2_EINVAL and "OV2_FKF_MAX_POINTS" in str(err.value)
    big.close()


def _ckf_work_bytes(det_cell):
    """the single-scale detector's work block of a call (csrc: ckf_work): every item's output list, then one pass's response maps,
    candidates and free-cell lists, each range rounded up to 256 bytes"""
    up = lambda v: (v + 255) // 256 * 256
    nc = (W // det_cell) * (H // det_cell)
    return up(8 * 2 * nc * BATCH) + up(BATCH * nc * det_cell * det_cell * 4) + up(BATCH * nc * 16) + up(BATCH * 4 * (nc + 1))


def _views(t):
    return dict(device=[RR.frame_bytes(t.getFrame(b, True)) for b in range(BATCH)], mirror=[RR.frame_bytes(t.getFrame(b, False)) for b in range(BATCH)],
                info_device=[t.getKeyframeInfo(b, True) for b in range(BATCH)], info_mirror=[t.getKeyframeInfo(b, False) for b in range(BATCH)])


def _grow_play(ctx, small_first):
    """frame 0, [a call that flags nobody with a detector cell of 64: the work block at its size], round 0 of the scenario, and a
    trackMono step on frame 1 that reads the keyframes the round installed"""
    cal = _cal(ctx)
    t = _tracker(ctx, cal)
    for b in range(BATCH):
        t.setPose(b, _truth(b)[0])
    a, kw = _mono_args(cal, 0, [None] * BATCH)
    _mono_step(t, a, kw)
    for b in range(BATCH):
        t.setPose(b, _truth(b)[0])
    state = _state0("singlescale")
    if small_first:
        x, p = CC.round_inputs(0), dict(CC.round_params(CC.ROUNDS[0], "singlescale"), det_cell=64)
        before, out = _views(t), _poison()
        recs, out = t.createKeyframe(4, x["px"], x["lmid"], x["is3d"], x["n"], np.zeros(BATCH, np.uint8), x["nlmid"], x["nkfid"], x["time"], p,
                                     state, Twc=x["Twc"], out=out)
        assert [r["action"] for r in recs] == [L.OV2_CKF_NOT_REQUESTED] * 4
        assert state.tobytes() == _state0("singlescale").tobytes() and all(out[k].tobytes() == v.tobytes() for k, v in _poison().items())
        assert _views(t) == before
    recs, out = _round(ctx, t, cal, 0, "singlescale", "fused", state)
    res = dict(recs=recs, out=out, state=state.copy(), views=_views(t))
    kf = [(out["px"][b, :r["n_kf"]].copy(), out["lmid"][b, :r["n_kf"]].copy()) if r["action"] == L.OV2_CKF_CREATED else None for b, r in enumerate(recs)]
    t.setPose(1, _invert(_wrong(_invert(_truth(1)[1]), np.random.default_rng(41), float(cal.K[0]))))          # item 1: the rule fires
    a, kw = _mono_args(cal, 1, kf)
    res["step"] = _mono_step(t, a, kw)
    res["views_after"] = _views(t)
    t.close()
    return res


def test_a_grown_work_block_changes_nothing(gpu_ctx):
    """The detector's work block is grow-only.  Tracker A's first call flags nobody and asks for a detector cell of 64, whose work block
    is smaller than the scenario's: it changes nothing (records, outputs, adaptive state, frames, keyframe info) and A's scenario round
    then grows the block.  Tracker B plays the round alone on a block allocated at that size.  Records, every output array, the adaptive
    state, the frames and the keyframe info from the device and from the mirror, and the trackMono step that reads the installed
    keyframes (the rule fires on item 1: the host re-run reads their mirror) are byte-equal."""
    assert 0 < _ckf_work_bytes(64) < _ckf_work_bytes(CC.BASE["det_cell"])
    A, B = _grow_play(gpu_ctx, True), _grow_play(gpu_ctx, False)
    _same_round(A, B, "grown work block")
    assert [r["action"] for r in A["recs"]] == [L.OV2_CKF_CREATED] * 4 and all(r["n_new"] > 0 for r in A["recs"])
    assert A["views"] == B["views"] and A["views"]["info_device"] == A["views"]["info_mirror"]
    _same_mono_step(A["step"], B["step"], "the step after the grown block")
    assert A["step"]["rule"][1]
    assert A["views_after"] == B["views_after"]
