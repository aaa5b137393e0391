"""The lock-step step with epipolar2d2dFiltering and the pose fused in (ov2_btracker_track_frame_epi_pose; csrc/trackb.hip,
csrc/frameepi.hip, csrc/epifilter.hip, csrc/framepose.hip) against the separate calls it replaces (tests/frameepi_ref.py: route).
Tracker A plays a sequence through route(), tracker B through the fused step; EVERY comparison is on raw bytes: both sides run the
same device kernels on the same inputs, and the chain's bits do not depend on the block's layout (OV2_OPT_EPIF_CAPACITY in
tests/test_gpu_epifilter.py), so equality is the derived requirement, not a tolerance.

Shapes as tests/test_gpu_framepose.py: 376 x 240, batch 3, 64 slots, four tracked frames, no CLAHE.  As there, every step draws fresh
keypoints and gives them map points that project onto the true track under the true pose.  The keyframe of a step is that cloud seen
from a second camera (x_kf = R x_cur + t, about 0.35 m to the side): its unpx / bv are exact projections, its ids are the slots'
lmids in ascending order, a few slots have no counterpart and the keyframe holds a few entries of its own.  Outliers are planted in
the ids alone -- two slots swap their lmid, or a slot points at one of the keyframe's own entries --, so the map points stay right and
the pose step without the filter (f16, played beside) keeps those keypoints in its pose set."""
import ctypes as C

import numpy as np
import pytest

import ov2slam_amd
from ov2slam_amd import _lib as L
from ov2slam_amd import keyframe, lockstep, pose
from tests import camera_cases as CC
from tests import fivept_ref as E5
from tests import frameepi_ref as R
from tests import framepose_ref as F
from tests import kfreq_ref as KF
from tests.epifilter_ref import _aa, _q_of
from tests.match_ref import _inv_act, _rand_pose
from tests.test_gpu_framepose import _invert, _near, _params, _same_step
from tests.test_gpu_priors_lockstep import BATCH, DIST, H, K, N_MAX, W, _wrong
from tests.test_gpu_tracker import _bits, _sequence

pytestmark = pytest.mark.gpu

I7 = np.array([0, 0, 0, 0, 0, 0, 1.0])
EPI_ROWS = 48


def _epi_params(stereo, mono, n_rows=EPI_ROWS, Kc=K):
    return dict(fkf=KF.make_params(K=Kc, img_w=W, img_h=H, stereo=stereo), max_iterations=100, threshold=E5.threshold_of(3.0, Kc[0], Kc[1]),
                probability=0.99, fransac_err=3.0, mono=mono, n_rows=n_rows)


# One step of a sequence.  Per item: counts keypoints, of which a share 0.75 (or exactly n3d[b]) is 3-D; swap3 / swap2: pairs of 3-D /
# 2-D slots that swap their lmid; point3: 3-D slots pointed at an entry of the keyframe's own; frac: that share of ALL slots pointed at
# such entries; kf: "ok", "same" (the keyframe is the frame itself: no parallax), "none" (taken away), "disjoint" (shares no id).
#   stereo: 0  more than 30 3-D keypoints (the join takes the 3-D ones, the Sampson pass the 2-D ones) / fewer than 31 (the join takes
#              all) / no keypoints
#           1  five 3-D keypoints of which two are planted, five of which one is planted, fewer than 8 keypoints
#           2  the frame repeated and the keyframe equal to it: LOW_PARALLAX
#           3  more than half planted: DEGENERATE; no keyframe; a keyframe that shares no id
#   mono:   0  nbkfs 3 and fewer than 30 3-D keypoints: pose_from_model; dop3p under LMedS
#           1  dop3p under RANSAC, nbkfs 2 on one item
#           2  the wrong motion model: the rule fires
#           3  the third item has ended; p3p_req on one item
#   grow:   the pose's sample rows go 7, 40 and the filter's (epi_rows) 8, 48 on one tracker, P3P and the five-point search running in
#           both steps: the second step grows the chain's work block and the filter's block behind a finished step, and the filter's
#           block gets the resident keyframe arrays again from the host copy
STEREO = [dict(counts=[64, 37, 0], swap3=[2, 1, 0], swap2=[2, 0, 0], scale=True),
          dict(counts=[20, 20, 6], n3d=[5, 5, 3], point3=[2, 1, 0], req=[1, 1, 1], n_rows=40, exact=True),
          dict(counts=[64, 37, 0], kf=["same", "same", "same"], repeat=True),
          dict(counts=[64, 37, 40], frac=[0.6, 0, 0], kf=["ok", "none", "disjoint"])]
MONO = [dict(counts=[64, 37, 0], n3d=[20, 10, 0], point3=[3, 2, 0], dop3p=True, n_rows=40),
        dict(counts=[37, 0, 64], n3d=[12, 0, 25], swap3=[1, 0, 2], dop3p=True, n_rows=40, mode=pose.RANSAC, nbkfs=[3, 3, 2]),
        dict(counts=[0, 64, 37], wrong_pose=True, n_rows=40, swap3=[0, 2, 1]),
        dict(counts=[64, 37], req=[0, 1], n_rows=7, scale=True, swap3=[1, 1])]
GROW = [dict(counts=[64, 37, 0], n3d=[20, 10, 0], point3=[3, 2, 0], dop3p=True, n_rows=7, epi_rows=8),
        dict(counts=[37, 20, 64], n3d=[12, 8, 25], swap3=[1, 0, 2], dop3p=True, n_rows=40, epi_rows=48)]
SPECS = dict(stereo=(STEREO, dict(stereo=True, mono=False)), mono=(MONO, dict(stereo=False, mono=True)),
             grow=(GROW, dict(stereo=False, mono=True)))

_SEQS, _RUNS = {}, {}


def _seqs():
    if not _SEQS:
        _SEQS["s"] = [_sequence(W, H, 5, seed=70 + b) for b in range(BATCH)]
    return _SEQS["s"]


def _rot_of(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _keyframe(rng, T, Pc, ids, pointed, planted, mode, Kc=K):
    """the cloud Pc (points in the current camera, whose world-to-camera pose is T) seen from the keyframe's camera.  ids: the id of
    the map point each slot REALLY shows; pointed: slot -> the id it carries instead (an entry of the keyframe's own, somewhere in the
    image); planted: slots that must keep their counterpart.  -> dict(lmid ascending, unpx, bv, Twc), at most N_MAX entries"""
    fx, fy, cx, cy = Kc
    m = len(Pc)
    same = mode == "same"
    Rrel = np.eye(3) if same else _aa(np.array([0.02, -0.03, 0.01]) * rng.uniform(0.6, 1.4))
    trel = np.zeros(3) if same else np.array([0.35, 0.05, 0.1]) * rng.uniform(0.8, 1.3)
    Rcw = _rot_of(T[3:])
    Rwc, twc = Rcw.T, -Rcw.T @ T[:3]
    Rwk = Rwc @ Rrel.T
    Twk = np.concatenate([twc - Rwk @ trel, _q_of(Rwk)])
    Pk = Pc @ Rrel.T + trel
    known = np.ones(m, bool)
    free = np.nonzero(~planted)[0]
    known[rng.permutation(free)[:min(3, m // 8)]] = False            # a few slots without a counterpart
    known[list(pointed)] = False                                      # (their own map points are not in the keyframe)
    n_own = len(pointed) + min(3, N_MAX - int(known.sum()) - len(pointed))
    own_ids = np.array(sorted(pointed.values()) + [200000 + j for j in range(n_own - len(pointed))], np.int32)
    own = np.stack([(rng.uniform(30, W - 30, n_own) - cx) / fx, (rng.uniform(30, H - 30, n_own) - cy) / fy, np.ones(n_own)], 1)
    kid = np.concatenate([ids[known], own_ids]).astype(np.int32)
    P = np.concatenate([Pk[known], own.reshape(-1, 3)])
    if mode == "disjoint":
        kid = kid + 500000
    o = np.argsort(kid)
    kid, P = kid[o], P[o]
    assert len(kid) <= N_MAX and (np.diff(kid) > 0).all()
    un = np.stack([fx * P[:, 0] / P[:, 2] + cx, fy * P[:, 1] / P[:, 2] + cy], 1).astype(np.float32)
    return dict(lmid=kid, unpx=un, bv=P / np.linalg.norm(P, axis=1)[:, None], Twc=Twk)


def _inputs(name, cal):
    """the per-step arguments of a sequence (a function of the name alone)"""
    seqs, rng, steps = _seqs(), np.random.default_rng(len(name) + 41), []
    spec, cfg = SPECS[name]
    Kc = tuple(float(v) for v in cal.K)
    prev_idx = 0
    for f, sp in enumerate(spec):
        cur_idx = prev_idx if sp.get("repeat") else prev_idx + 1
        na = len(sp["counts"])
        kps = np.zeros((BATCH, N_MAX, 2), np.float32); wpt = np.zeros((BATCH, N_MAX, 3)); is3d = np.zeros((BATCH, N_MAX), np.uint8)
        lmid = np.zeros((BATCH, N_MAX), np.int32)
        Tcw, Twc = np.tile(I7, (BATCH, 1)), np.tile(I7, (BATCH, 1))
        n = np.array(sp["counts"], np.int32)
        kfs = []
        for b in range(na):
            m = int(n[b])
            mode = sp.get("kf", ["ok"] * na)[b]
            k = np.stack([rng.uniform(20, W - 20, m), rng.uniform(20, H - 20, m)], 1).astype(np.float32)
            true = seqs[b][1](k.astype(np.float64), prev_idx, cur_idx)
            gt = (true + rng.normal(0, 0.0 if sp.get("exact") else 0.3, (m, 2))).astype(np.float32)
            T = _rand_pose(rng)
            if "n3d" in sp:
                d3 = np.zeros(m, np.uint8); d3[rng.permutation(m)[:sp["n3d"][b]]] = 1
            else:
                d3 = (rng.uniform(size=m) < 0.75).astype(np.uint8)
            bv = cal.computeKeypoints(gt)[1] if m else np.zeros((0, 3))
            Pc = np.array([bv[i] / bv[i][2] * rng.uniform(2, 10) for i in range(m)]).reshape(m, 3)
            for i in range(m):
                wpt[b, i] = _inv_act(T, Pc[i])
            real = (10 + 3 * rng.permutation(m)).astype(np.int32)     # a shuffled map order
            ids = real.copy()
            # the plants: in the ids alone
            three, two = rng.permutation(np.nonzero(d3)[0]), rng.permutation(np.nonzero(d3 == 0)[0])
            s3, s2, p3 = (sp.get(key, [0] * na)[b] for key in ("swap3", "swap2", "point3"))
            planted, pointed = np.zeros(m, bool), {}
            for x, c in list(zip(three[:2 * s3:2], three[1:2 * s3:2])) + list(zip(two[:2 * s2:2], two[1:2 * s2:2])):
                ids[x], ids[c] = real[c], real[x]
                planted[[x, c]] = True
            nfr = int(round(sp.get("frac", [0] * na)[b] * m))
            for x in list(three[2 * s3:2 * s3 + p3]) + list(rng.permutation(m)[:nfr]):
                pointed[int(x)] = ids[x] = 100000 + len(pointed)
            kf = None if mode == "none" else _keyframe(rng, T, Pc, real, pointed, planted, mode, Kc)
            kps[b, :m], is3d[b, :m], lmid[b, :m] = k, d3, ids
            Tp = _wrong(T, rng, Kc[0]) if sp.get("wrong_pose") else _near(T, rng)
            Tcw[b], Twc[b] = Tp, _invert(Tp)
            kfs.append(kf)
        req = np.zeros(BATCH, np.uint8); req[:na] = sp.get("req", [0] * na)
        nbkfs = np.full(BATCH, 3, np.int32); nbkfs[:na] = sp.get("nbkfs", [3] * na)
        steps.append(dict(imgs=[seqs[b][0][cur_idx] for b in range(na)], kps=kps, wpt=wpt, is3d=is3d, Tcw=Tcw, n=n, Twc=Twc, p3p_req=req,
                          seed=rng.integers(0, 1 << 63, BATCH).astype(np.uint64) * np.uint64(2) + np.uint64(1),
                          epi_seed=rng.integers(0, 1 << 63, BATCH).astype(np.uint64) * np.uint64(2) + np.uint64(1),
                          lmid=lmid, nbkfs=nbkfs, keyframes=kfs,
                          scale=rng.integers(0, 4, (BATCH, N_MAX)).astype(np.int32) if sp.get("scale") else None,
                          params=_params(sp.get("mode", pose.LMEDS), cfg["mono"], Kc),
                          epi_params=_epi_params(cfg["stereo"], cfg["mono"], sp.get("epi_rows", EPI_ROWS), Kc),
                          dop3p=sp.get("dop3p", False), n_rows=sp.get("n_rows", 0), klt_use_prior=True))
        prev_idx = cur_idx
    return steps


def _tracker(ctx, cal):
    t = ov2slam_amd.LockstepTracker(ctx, BATCH, W, H, use_clahe=False, nbmaxkps=N_MAX)
    t.setCalibration(cal)
    return t


def _epi_call(t, s, **over):
    a = (s["imgs"], s["kps"], s["wpt"], s["is3d"], s["Tcw"], s["n"])
    kw = dict(scale=s["scale"], dop3p=s["dop3p"], n_rows=s["n_rows"], klt_use_prior=s["klt_use_prior"])
    kw.update(over)
    return a, (s["params"], s["epi_params"], s["Twc"], s["p3p_req"], s["seed"], s["lmid"], s["nbkfs"], s["epi_seed"]), kw


def _first(t, how):
    z2, z3, z1 = np.zeros((BATCH, N_MAX, 2), np.float32), np.zeros((BATCH, N_MAX, 3)), np.zeros((BATCH, N_MAX), np.uint8)
    first = [_seqs()[b][0][0] for b in range(BATCH)]
    zn, T = np.zeros(BATCH, np.int32), np.tile(I7, (BATCH, 1))
    if how == "route":
        return t.trackFrameMap(first, z2, z3, z1, T, zn)
    if how == "f16":
        return t.trackFramePose(first, z2, z3, z1, T, zn, _params(), T, np.zeros(BATCH, np.uint8), np.arange(BATCH, dtype=np.uint64))
    return t.trackFrameEpiPose(first, z2, z3, z1, T, zn, _params(), _epi_params(True, False), T, np.array([0, 1, 0], np.uint8),
                               np.arange(BATCH, dtype=np.uint64), np.zeros((BATCH, N_MAX), np.int32), np.zeros(BATCH, np.int32),
                               np.arange(BATCH, dtype=np.uint64))


def _set_keyframes(t, s):
    for b, kf in enumerate(s["keyframes"]):
        if kf is None:
            t.setKeyframe(b, np.zeros(0, np.int32), np.zeros((0, 2), np.float32), np.zeros((0, 3)), None)
        else:
            t.setKeyframe(b, kf["lmid"], kf["unpx"], kf["bv"], kf["Twc"])


def _call(t, s, how, ctx):
    a, e, kw = _epi_call(t, s)
    na = len(s["imgs"])
    epis = einputs = None
    if how == "route":
        out, st, rule, epis, poses, einputs, inputs = R.route(ctx, t, *a, *e, s["keyframes"], **kw)
    elif how == "f16":
        out, st, rule, poses = t.trackFramePose(*a, s["params"], s["Twc"], s["p3p_req"], s["seed"], **kw)
        inputs = [t.lastPoseInputs(b) for b in range(na)]
    else:
        _set_keyframes(t, s)
        if how == "fused":
            out, st, rule, epis, poses = t.trackFrameEpiPose(*a, *e, **kw)
        else:
            t.trackFrameEpiPoseBegin(*a, *e, **kw)
            out, st, rule, epis, poses = t.trackFrameEpiPoseEnd()
        inputs = [t.lastPoseInputs(b) for b in range(na)]
        einputs = [t.lastEpiInputs(b) for b in range(na)]
    kp = [t.lastKeypoints(b, int(s["n"][b])) for b in range(na)]
    pr = [t.lastPriors(b, int(s["n"][b])) for b in range(na)]
    return dict(out=out, st=st, rule=rule, poses=poses, inputs=inputs, kp=kp, pr=pr, epis=epis, einputs=einputs)


def _play(ctx, name, how, camera=None):
    """the sequence `name` on a fresh tracker, through route() ('route'), the one-call fused step ('fused'), its two halves ('halves')
    or the pose step without the filter ('f16'), under the EuRoC calibration or a camera of tests/camera_cases.py.  Computed once per
    (name, how, camera) and shared between the tests; nobody changes a result."""
    key = (name, how) if camera is None else (name, how, camera)
    if key not in _RUNS:
        cal = CC.calibration(ctx, camera) if camera else ov2slam_amd.CameraCalibration(ctx, "pinhole", *K, D=DIST)
        t = _tracker(ctx, cal)
        _first(t, how if how in ("route", "f16") else "fused")
        _RUNS[key] = [_call(t, s, how, ctx) for s in _inputs(name, cal)]
        t.close()
    return _RUNS[key]


def _same_epi_step(a, b, where):
    _same_step(a, b, where)                                       # tracking, keypoints, priors, poses, lastPoseInputs
    assert len(a["epis"]) == len(b["epis"])
    for i, (x, y) in enumerate(zip(a["epis"], b["epis"])):
        bx, by = R.epi_bytes(x), R.epi_bytes(y)
        for k in bx:
            assert bx[k] == by[k], (where, "item %d" % i, k, x["action"], y["action"])
    for i, (x, y) in enumerate(zip(a["einputs"], b["einputs"])):
        assert x[0] == y[0] and np.array_equal(x[1], y[1]) and x[2] == y[2] and np.array_equal(x[3], y[3]), (where, i, "lastEpiInputs")


def _show(name, A):
    for f, a in enumerate(A):
        print(name, f, [(e["action"], e["m"], e["nb3dkps"], e["n_removed_ransac"], e["n_removed_sampson"], e["pose_from_model"],
                         pose.ACTION_NAMES[p["action"]], i[0], p["ran_p3p"]) for e, p, i in zip(a["epis"], a["poses"], a["inputs"])],
              "rule", a["rule"].astype(int).tolist())


@pytest.mark.parametrize("name", sorted(SPECS))
def test_fused_step_equals_the_route(gpu_ctx, name):
    A, B = _play(gpu_ctx, name, "route"), _play(gpu_ctx, name, "fused")
    _show(name, A)
    for f, (a, b) in enumerate(zip(A, B)):
        _same_epi_step(a, b, (name, f))


@pytest.mark.parametrize("camera", CC.ADDED)
def test_fused_step_equals_the_route_under_added_cameras(gpu_ctx, oracle, camera):
    """The stereo sequence under the added cameras of tests/camera_cases.py: fused against route byte for byte, and after every step
    every item is tied to the reference (camera_cases.assert_step_anchor: lastKeypoints == ov2_compute_keypoints as bits == the
    oracle within the camera's bound; lastPriors == ov2_klt_priors_batch as bits)."""
    cal = CC.calibration(gpu_ctx, camera)
    steps = _inputs("stereo", cal)
    A, B = _play(gpu_ctx, "stereo", "route", camera), _play(gpu_ctx, "stereo", "fused", camera)
    _show(camera, A)
    assert len(A) == len(B) == len(steps)
    for f, (s, a, b) in enumerate(zip(steps, A, B)):
        _same_epi_step(a, b, (camera, f))
        CC.assert_step_anchor(gpu_ctx, oracle, cal, camera, s, b)
    # the filter still filters and the pose still solves under this camera
    assert A[0]["epis"][0]["action"] == keyframe.EPIF_FILTERED and A[0]["poses"][0]["action"] == pose.POSE_OK


def test_the_route_exercises_what_the_cases_are_for(gpu_ctx):
    """on the route's side alone: the sequences reach the actions and removal codes they were built for"""
    S, M, P16 = _play(gpu_ctx, "stereo", "route"), _play(gpu_ctx, "mono", "route"), _play(gpu_ctx, "stereo", "f16")
    cal = ov2slam_amd.CameraCalibration(gpu_ctx, "pinhole", *K, D=DIST)
    st_in, mo_in = _inputs("stereo", cal), _inputs("mono", cal)
    _show("stereo", S); _show("mono", M)
    # more than 30 3-D keypoints under stereo: the join takes the 3-D ones; planted 3-D mismatches go with code 1 and leave the pose
    # set (m below f16's on the same frame), planted 2-D mismatches go with code 2
    e, p = S[0]["epis"][0], S[0]["poses"][0]
    assert e["action"] == keyframe.EPIF_FILTERED and e["epifrom3dkps"] == 1 and e["nb3dkps"] > 30
    assert e["n_removed_ransac"] >= 3 and (e["removed"] == 1).sum() == e["n_removed_ransac"]
    assert e["n_removed_sampson"] >= 3 and (e["removed"] == 2).sum() == e["n_removed_sampson"]
    assert st_in[0]["is3d"][0][:64][e["removed"] == 1].all() and not st_in[0]["is3d"][0][:64][e["removed"] == 2].any()
    assert S[0]["inputs"][0][0] == P16[0]["inputs"][0][0] - e["n_removed_ransac"] and p["action"] == pose.POSE_OK
    assert not np.isin(np.nonzero(e["removed"])[0], S[0]["inputs"][0][1]).any()
    # fewer than 31: the join takes all keypoints
    e = S[0]["epis"][1]
    assert e["action"] == keyframe.EPIF_FILTERED and e["epifrom3dkps"] == 0 and e["nb3dkps"] < 31 and e["m"] > e["nb3dkps"]
    assert e["n_removed_ransac"] >= 2 and e["n_removed_sampson"] == 0
    assert S[0]["epis"][2]["action"] == keyframe.EPIF_TOO_FEW_KPS and S[0]["einputs"][2][0] == 0
    # five 3-D keypoints, two planted: three are left, TOO_FEW; one planted: four, P3P's boundary
    assert [i[0] for i in P16[1]["inputs"]] == [5, 5, 3]
    assert [e["action"] for e in S[1]["epis"]] == [keyframe.EPIF_FILTERED, keyframe.EPIF_FILTERED, keyframe.EPIF_TOO_FEW_KPS]
    assert [i[0] for i in S[1]["inputs"]] == [3, 4, 3]
    assert S[1]["poses"][0]["action"] == pose.TOO_FEW and not S[1]["poses"][0]["ran_p3p"] and S[1]["poses"][1]["ran_p3p"]
    assert S[1]["einputs"][2][0] == 6 and len(S[1]["einputs"][2][3]) == 0
    # a repeated frame: LOW_PARALLAX, nothing removed, the pose is f16's
    for b in (0, 1):
        e = S[2]["epis"][b]
        assert e["action"] == keyframe.EPIF_LOW_PARALLAX and e["parallax"] < 6 and not e["removed"].any() and e["m"] >= 8
        assert F.pose_bytes(S[2]["poses"][b]) == F.pose_bytes(P16[2]["poses"][b])
    # more than half planted: DEGENERATE, nothing removed; no keyframe and a keyframe that shares no id: NO_MODEL with a NaN parallax
    e = S[3]["epis"][0]
    assert e["action"] == keyframe.EPIF_DEGENERATE and e["n_outliers"] > 0.5 * e["m"] and not e["removed"].any()
    assert F.pose_bytes(S[3]["poses"][0]) == F.pose_bytes(P16[3]["poses"][0])
    for b in (1, 2):
        e = S[3]["epis"][b]
        assert e["action"] == keyframe.EPIF_NO_MODEL and e["m"] == 0 and np.isnan(e["parallax"]) and not e["removed"].any()
    # mono, nbkfs 3, fewer than 30 3-D keypoints: the pose of the unrefined model is reported; nbkfs 2: it is not
    for b in (0, 1):
        e = M[0]["epis"][b]
        assert e["action"] == keyframe.EPIF_FILTERED and e["do_optimize"] == 1 and e["pose_from_model"] == 1 and e["Twc_model"].any()
        assert e["n_removed_ransac"] >= 1
    assert M[1]["epis"][2]["do_optimize"] == 0 and M[1]["epis"][2]["pose_from_model"] == 0
    # dop3p under both modes: every item with four 3-D keypoints left searches
    for f in (0, 1):
        assert [p["ran_p3p"] for p in M[f]["poses"]] == [i[0] >= 4 for i in M[f]["inputs"]] and sum(i[0] >= 4 for i in M[f]["inputs"]) == 2
    # the wrong motion model: the rule fires on every item with keypoints and the second run filters and searches
    assert M[2]["rule"].tolist() == [False, True, True] and (M[2]["st"] & 2).any()
    assert all(p["ran_p3p"] for p in M[2]["poses"][1:]) and all(e["m"] >= 8 for e in M[2]["epis"][1:])
    # an item that has ended, p3p_req on one of the others
    assert len(M[3]["epis"]) == 2 and [p["ran_p3p"] for p in M[3]["poses"]] == [False, True]
    # grow: both searches run in both steps, on tables of 7 / 8 rows and then of 40 / 48
    G = _play(gpu_ctx, "grow", "route")
    _show("grow", G)
    for g, (prow, erow) in zip(G, ((7, 8), (40, 48))):
        assert sum(bool(p["ran_p3p"]) and len(i[2]) == prow for p, i in zip(g["poses"], g["inputs"])) >= 2
        assert sum(e["action"] == keyframe.EPIF_FILTERED and len(ei[3]) == erow for e, ei in zip(g["epis"], g["einputs"])) >= 2
    # every action and both removal codes were seen; removed speaks of slots of the frame, the pose's of slots of the filtered frame
    seen = {e["action"] for run in (S, M) for s in run for e in s["epis"]}
    assert seen == {keyframe.EPIF_TOO_FEW_KPS, keyframe.EPIF_LOW_PARALLAX, keyframe.EPIF_NO_MODEL, keyframe.EPIF_DEGENERATE, keyframe.EPIF_FILTERED}
    for run in (S, M):
        for s in run:
            for e, p, ei, pi in zip(s["epis"], s["poses"], s["einputs"], s["inputs"]):
                outside = np.ones(len(e["removed"]), bool); outside[ei[1]] = False
                assert not e["removed"][outside].any() and not p["removed"][e["removed"] != 0].any()
                assert np.isin(e["pair_cur"], ei[1]).all() and len(e["pair_cur"]) == e["m"]


def test_last_epi_inputs_are_the_packed_frame_and_the_host_draw(gpu_ctx):
    """lastEpiInputs of the fused step against frame_set and ov2_epipolar_draw_samples directly (not through the route)"""
    seen = 0
    for name in sorted(SPECS):
        B = _play(gpu_ctx, name, "fused")
        cal = ov2slam_amd.CameraCalibration(gpu_ctx, "pinhole", *K, D=DIST)
        for f, (s, r) in enumerate(zip(_inputs(name, cal), B)):
            for b, (n_cur, slots, m, tab) in enumerate(r["einputs"]):
                want = R.frame_set(r["st"][b], int(s["n"][b]))
                assert n_cur == len(want) and np.array_equal(slots, want) and m == r["epis"][b]["m"], (name, f, b)
                search = r["epis"][b]["action"] >= keyframe.EPIF_NO_MODEL and m >= 8
                rows = s["epi_params"]["n_rows"]                   # (EPI_ROWS wherever the spec does not say otherwise)
                assert len(tab) == (rows if search else 0), (name, f, b)
                if search:
                    assert np.array_equal(tab, pose.epipolar_draw_samples(int(s["epi_seed"][b]), m, rows)), (name, f, b)
                seen += bool(search)
    assert seen >= 10


def test_begin_end_equals_the_one_call_form(gpu_ctx):
    for f, (a, b) in enumerate(zip(_play(gpu_ctx, "mono", "fused"), _play(gpu_ctx, "mono", "halves"))):
        _same_epi_step(a, b, ("halves", f))


def test_a_second_run_on_fresh_trackers_gives_the_same_bytes(gpu_ctx):
    first = _play(gpu_ctx, "stereo", "fused")
    del _RUNS[("stereo", "fused")]
    try:
        again = _play(gpu_ctx, "stereo", "fused")
    finally:
        _RUNS[("stereo", "fused")] = first
    for f, (a, b) in enumerate(zip(first, again)):
        _same_epi_step(a, b, ("repeat", f))


def test_first_frame_and_empty_step_run_nothing(gpu_ctx):
    cal = ov2slam_amd.CameraCalibration(gpu_ctx, "pinhole", *K, D=DIST)
    t = _tracker(gpu_ctx, cal)                                    # no keyframe is ever set on this tracker
    Twc = np.stack([_rand_pose(np.random.default_rng(b)) for b in range(BATCH)])
    req = np.array([0, 1, 0], np.uint8)
    z2, z3, z1 = np.zeros((BATCH, N_MAX, 2), np.float32), np.zeros((BATCH, N_MAX, 3)), np.zeros((BATCH, N_MAX), np.uint8)
    seqs = _seqs()
    for f, n in enumerate(([5, 0, 9], [0, 0, 0])):                # the first frame (with keypoints passed), then a step that tracks nothing
        out, st, rule, epis, poses = t.trackFrameEpiPose([seqs[b][0][f] for b in range(BATCH)], z2 + 50, z3 + 1, z1 + 1, np.tile(I7, (BATCH, 1)),
                                                         n, _params(), _epi_params(True, False), Twc, req, np.arange(BATCH, dtype=np.uint64),
                                                         np.zeros((BATCH, N_MAX), np.int32), np.full(BATCH, 3, np.int32),
                                                         np.arange(BATCH, dtype=np.uint64), dop3p=True, n_rows=10)
        assert not st.any() and not rule.any()
        for b in range(BATCH):
            assert F.pose_bytes(F.nothing_ran(Twc[b], req[b], n[b])) == F.pose_bytes(poses[b]), (f, b)
            assert R.epi_bytes(R.nothing_ran(n[b])) == R.epi_bytes(epis[b]), (f, b)
            assert t.lastEpiInputs(b)[0] == 0 and len(t.lastEpiInputs(b)[3]) == 0 and t.lastPoseInputs(b)[0] == 0
    t.close()


def test_rejected_calls_leave_outputs_and_tracker_untouched(gpu_ctx):
    """every refusal is OV2_EINVAL before anything is enqueued; the next valid step equals tracker A's; setKeyframe is refused while a
    step is open; a step begun with the epipolar form and finished with the plain end call gives the tracking half and drops both
    results"""
    cal = ov2slam_amd.CameraCalibration(gpu_ctx, "pinhole", *K, D=DIST)
    steps, A = _inputs("stereo", cal), _play(gpu_ctx, "stereo", "route")
    s = steps[0]
    a, e, kw = _epi_call(None, s)
    t = ov2slam_amd.LockstepTracker(gpu_ctx, BATCH, W, H, use_clahe=False, nbmaxkps=N_MAX)
    with pytest.raises(ov2slam_amd.Ov2Error) as err:              # no calibration
        t.trackFrameEpiPose(*a, *e, **kw)
    assert err.value.code == L.OV2_EINVAL and "calibration" in str(err.value)
    t.setCalibration(cal)
    _first(t, "fused")
    # the keyframe's own refusals
    kf = s["keyframes"][0]
    nan_bv = kf["bv"].copy(); nan_bv[2, 1] = np.nan
    for args in ((kf["lmid"][::-1], kf["unpx"], kf["bv"], kf["Twc"]), (kf["lmid"], kf["unpx"], nan_bv, kf["Twc"]),
                 (kf["lmid"], kf["unpx"], kf["bv"], np.where(np.arange(7) == 1, np.inf, kf["Twc"])),
                 (np.arange(N_MAX + 1), np.zeros((N_MAX + 1, 2)), np.ones((N_MAX + 1, 3)), kf["Twc"])):
        with pytest.raises(ov2slam_amd.Ov2Error) as err:
            t.setKeyframe(0, *args)
        assert err.value.code == L.OV2_EINVAL
    with pytest.raises(ov2slam_amd.Ov2Error) as err:
        t.setKeyframe(BATCH, kf["lmid"], kf["unpx"], kf["bv"], kf["Twc"])
    assert err.value.code == L.OV2_EINVAL
    assert t.lib.ov2_btracker_set_keyframe(t.h_trk, 0, 3, None, None, None, None) == L.OV2_EINVAL
    # the step's refusals: the pose step's, the filter's, and its own
    sc61 = np.zeros((BATCH, N_MAX), np.int32); sc61[0, 3] = 61
    bad = [dict(n_rows=L.OV2_P3P_MAX_ROWS + 1), dict(scale=sc61), dict(epi=dict(n_rows=L.OV2_EPI_MAX_ROWS + 1)), dict(epi=dict(n_rows=-1)),
           dict(epi=dict(boptimize=True)), dict(epi=dict(probability=1.0)), dict(epi=dict(threshold=0.0)), dict(epi=dict(max_iterations=-1))]
    for k in bad:
        ep = dict(s["epi_params"], **k.pop("epi", {}))
        with pytest.raises(ov2slam_amd.Ov2Error) as err:
            t.trackFrameEpiPose(*a, e[0], ep, *e[2:], **dict(kw, **k))
        assert err.value.code == L.OV2_EINVAL, ep
    # NULL lmid_h / nbkfs_h / epi_seed_h through the C ABI, with poisoned outputs: nothing is written
    for field in ("lmid_h", "nbkfs_h", "epi_seed_h"):
        c = t._marshal_track_frame_epi_pose(*a, *e)
        setattr(c.inputs, field, None)
        na = c.na
        out = np.full((BATCH, N_MAX, 2), 7.5, np.float32); st = np.full((BATCH, N_MAX), 0x6E, np.uint8); p3p = np.full(na, 0x6E6E, np.int32)
        res = lockstep._Results(t, "track_frame_epi_pose", c)
        Rp, removed, Re, bufs = res.R, res.removed, res.E, res.bufs
        removed[...] = 0x6E; bufs["removed"][...] = 0x6E
        before = bytes(C.string_at(C.byref(Rp), C.sizeof(Rp))) + bytes(C.string_at(C.byref(Re), C.sizeof(Re)))
        rc = t.lib.ov2_btracker_track_frame_epi_pose(t.h_trk, *c.args, out.ctypes.data, st.ctypes.data, p3p.ctypes.data, Re, Rp)
        assert rc == L.OV2_EINVAL and b"NULL" in t.lib.ov2_last_error(), field
        assert (out == 7.5).all() and (st == 0x6E).all() and (p3p == 0x6E6E).all() and (removed == 0x6E).all() and (bufs["removed"] == 0x6E).all()
        assert bytes(C.string_at(C.byref(Rp), C.sizeof(Rp))) + bytes(C.string_at(C.byref(Re), C.sizeof(Re))) == before
    # the tracker is where it was: the same frames pass now, and give what tracker A gave; the keyframe cannot change while a step is open
    _set_keyframes(t, s)
    t.trackFrameEpiPoseBegin(*a, *e, **kw)
    with pytest.raises(ov2slam_amd.Ov2Error) as err:
        t.setKeyframe(0, kf["lmid"], kf["unpx"], kf["bv"], kf["Twc"])
    assert err.value.code == L.OV2_EINVAL and "open" in str(err.value)
    # ... and a trace_samples pointer is refused by the end half, which leaves the step open
    res = lockstep._Results(t, "track_frame_epi_pose", c)
    Rp, Re = res.R, res.E
    tab = np.zeros((EPI_ROWS, 8), np.int32)
    Re[0].trace_samples = tab.ctypes.data_as(C.POINTER(C.c_int))
    out = np.zeros((BATCH, N_MAX, 2), np.float32); st = np.zeros((BATCH, N_MAX), np.uint8); p3p = np.zeros(na, np.int32)
    assert t.lib.ov2_btracker_track_frame_epi_pose_end(t.h_trk, out.ctypes.data, st.ctypes.data, p3p.ctypes.data, Re, Rp) == L.OV2_EINVAL
    assert t.lib.ov2_btracker_track_frame_pose_end(t.h_trk, out.ctypes.data, st.ctypes.data, p3p.ctypes.data, Rp) == L.OV2_EINVAL
    out, st, rule, epis, poses = t.trackFrameEpiPoseEnd()
    na = len(s["imgs"])
    got = dict(out=out, st=st, rule=rule, epis=epis, poses=poses, inputs=[t.lastPoseInputs(b) for b in range(na)],
               einputs=[t.lastEpiInputs(b) for b in range(na)], kp=[t.lastKeypoints(b, int(s["n"][b])) for b in range(na)],
               pr=[t.lastPriors(b, int(s["n"][b])) for b in range(na)])
    _same_epi_step(A[0], got, "after the refusals")
    # the epipolar form finished by the plain end call: the tracking half, neither result
    s1 = steps[1]
    _set_keyframes(t, s1)
    a1, e1, kw1 = _epi_call(t, s1)
    t.trackFrameEpiPoseBegin(*a1, *e1, **kw1)
    out, st, rule = t.trackFrameEnd()
    assert np.array_equal(_bits(out), _bits(A[1]["out"])) and np.array_equal(st, A[1]["st"]) and np.array_equal(rule, A[1]["rule"])
    got = _call(t, steps[2], "fused", gpu_ctx)
    _same_epi_step(A[2], got, "after the plain end call")
    t.close()


def test_capacity_beyond_the_filter_is_refused(gpu_ctx):
    t = ov2slam_amd.LockstepTracker(gpu_ctx, 1, 128, 128, use_clahe=False, nbmaxkps=L.OV2_FKF_MAX_POINTS + 1)
    with pytest.raises(ov2slam_amd.Ov2Error) as err:
        t.setKeyframe(0, np.zeros(0, np.int32), np.zeros((0, 2)), np.zeros((0, 3)), None)
    assert err.value.code == L.OV2_EINVAL and "n_max" in str(err.value)
    t.close()
