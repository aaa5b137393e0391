"""The lock-step step with the pose fused in (ov2_btracker_track_frame_pose; csrc/trackb.hip, csrc/framepose.hip, csrc/pnp.hip)
against the separate calls it replaces (tests/framepose_ref.py: route).  Tracker A plays a sequence through route(), tracker B through
the fused step; EVERY comparison is on raw bytes: a problem gives the same bits at any batch position and layout and the chain
equals its parts, so equality is the derived requirement, not a tolerance.

Shapes as tests/test_gpu_priors_lockstep.py: 376 x 240, batch 3, 64 slots, five frames, no CLAHE.  Map points project onto the true
track under the true pose; the predicted pose is the true one slightly disturbed, so that PnP has something to do."""
import numpy as np
import pytest

import ov2slam_amd
from ov2slam_amd import _lib as L
from ov2slam_amd import lockstep, pose
from tests import camera_cases as CC
from tests import framepose_ref as F
from tests.match_ref import _inv_act, _rand_pose
from tests.test_gpu_priors_lockstep import BATCH, DIST, H, K, N_MAX, NFRAMES, W, _wrong
from tests.test_gpu_tracker import _bits, _sequence

pytestmark = pytest.mark.gpu

COUNTS = [64, 37, 0]
I7 = np.array([0, 0, 0, 0, 0, 0, 1.0])


def _params(mode=pose.LMEDS, mono=False, Kc=K):
    return dict(pnp=dict(nmaxiter=5, chi2th=5.9915, use_robust=True, apply_l2_after_robust=True, K=np.array(Kc)),
                p3p=dict(mode=mode, max_iterations=40, threshold=pose.threshold(3.0, Kc[0], Kc[1]), probability=0.99, boptimize=False), mono=mono)


def _invert(T):
    """[t q] of the inverse transform"""
    x, y, z, w = T[3:]
    return np.concatenate([_inv_act(T, (0.0, 0.0, 0.0)), [-x, -y, -z, w]])


def _near(T, rng):
    """T disturbed by ~0.2 degrees and ~5 mm: the priors land within a pixel or two, PnP starts off the optimum"""
    a = rng.normal(0, 0.0035, 3)
    x, y, z, w = T[3:]
    dq = np.array([a[0] / 2, a[1] / 2, a[2] / 2, 1.0])
    q = np.array([dq[3] * x + dq[0] * w + dq[1] * z - dq[2] * y, dq[3] * y - dq[0] * z + dq[1] * w + dq[2] * x,
                  dq[3] * z + dq[0] * y - dq[1] * x + dq[2] * w, dq[3] * w - dq[0] * x - dq[1] * y - dq[2] * z])
    return np.concatenate([T[:3] + rng.normal(0, 0.005, 3), q / np.linalg.norm(q)])


# One step of a sequence: counts[b] keypoints per item, of which a share `frac3d` (or exactly n3d[b]) is 3-D.
#   main: the counts and the 3-D share; wrong map points (without klt priors: a prior 20 px off would send those keypoints through the
#         retry and out of the pose set); the wrong motion model (the rule fires); p3p_req on two items while the third has ended
#   alt:  dop3p on all in both search modes (mono once); the small 3-D counts 3 / 4 / 5; scales
MAIN = [dict(counts=[64, 37, 0], scale=True),
        dict(counts=[37, 0, 64], wrong_map=True, use_prior=False),
        dict(counts=[0, 64, 37], wrong_pose=True, n_rows=40),
        dict(counts=[64, 37], req=[1, 1], n_rows=40)]
ALT = [dict(counts=[64, 37, 0], dop3p=True, n_rows=40),
       dict(counts=[37, 0, 64], dop3p=True, n_rows=40, mode=pose.RANSAC, mono=True),
       dict(counts=[20, 20, 20], n3d=[3, 4, 5], req=[1, 1, 1], n_rows=40, exact=True),
       dict(counts=[64, 64, 64], req=[0, 1, 0], n_rows=7, scale=True)]
# fold: one step for the camera fisheye_fold (tests/camera_cases.py).  Half of the key points lie just beyond the radius at which its
#       undistortion fails and have map points that project next to them (camera_cases.fold_rays), so they track, and the pose set
#       carries (-1e6, -1e6) pixels and their bearings into P3P (requested on both items) and both PnP passes
FOLD = [dict(counts=[64, 37, 0], req=[1, 1, 0], n_rows=40, fold=True)]
SPECS = dict(main=MAIN, alt=ALT)
CAMERA_SPECS = dict(SPECS, fold=FOLD)

_SEQS, _RUNS = {}, {}


def _seqs():
    if not _SEQS:
        _SEQS["s"] = [_sequence(W, H, NFRAMES, seed=70 + b) for b in range(BATCH)]
    return _SEQS["s"]


def _inputs(name, cal):
    """the per-step arguments of a sequence (a function of the name alone)"""
    seqs, rng, steps = _seqs(), np.random.default_rng(len(name) + 23), []
    Kc = tuple(float(v) for v in cal.K)
    for f, sp in enumerate(CAMERA_SPECS[name]):
        na = len(sp["counts"])
        kps = np.zeros((BATCH, N_MAX, 2), np.float32); wpt = np.zeros((BATCH, N_MAX, 3)); is3d = np.zeros((BATCH, N_MAX), np.uint8)
        Tcw, Twc = np.tile(I7, (BATCH, 1)), np.tile(I7, (BATCH, 1))
        n = np.array(sp["counts"], np.int32)
        for b in range(na):
            m = int(n[b])
            k = np.stack([rng.uniform(20, W - 20, m), rng.uniform(20, H - 20, m)], 1).astype(np.float32)
            if sp.get("fold"):
                k = CC.fold_ring_points(m, rng)
            true = seqs[b][1](k.astype(np.float64), f, f + 1)
            gt = (true + rng.normal(0, 0.0 if sp.get("exact") else 0.3, (m, 2))).astype(np.float32)
            T = _rand_pose(rng)
            if "n3d" in sp:
                d3 = np.zeros(m, np.uint8); d3[rng.permutation(m)[:sp["n3d"][b]]] = 1
            else:
                d3 = (rng.uniform(size=m) < 0.75).astype(np.uint8)
            if sp.get("wrong_map"):                               # one in eight 3-D slots: a map point that projects ~20 px off, inside
                bad = np.nonzero(d3)[0][::8]
                gt[bad, 0] += np.where(gt[bad, 0] < W / 2, 20.0, -20.0).astype(np.float32)
            bv = cal.computeKeypoints(gt)[1] if m else np.zeros((0, 3))
            if sp.get("fold") and m:
                bv = CC.fold_rays(gt, bv)
            for i in range(m):
                wpt[b, i] = _inv_act(T, bv[i] / bv[i][2] * rng.uniform(2, 10))
            kps[b, :m], is3d[b, :m] = k, d3
            Tp = _near(T, rng)
            if sp.get("wrong_pose"):
                Tp = _wrong(T, rng, Kc[0])
            Tcw[b], Twc[b] = Tp, _invert(Tp)
        req = np.zeros(BATCH, np.uint8); req[:na] = sp.get("req", [0] * na)
        steps.append(dict(imgs=[seqs[b][0][f + 1] for b in range(na)], kps=kps, wpt=wpt, is3d=is3d, Tcw=Tcw, n=n, Twc=Twc, p3p_req=req,
                          seed=rng.integers(0, 1 << 63, BATCH).astype(np.uint64) * np.uint64(2) + np.uint64(1),
                          scale=rng.integers(0, 4, (BATCH, N_MAX)).astype(np.int32) if sp.get("scale") else None,
                          params=_params(sp.get("mode", pose.LMEDS), sp.get("mono", False), Kc), dop3p=sp.get("dop3p", False),
                          n_rows=sp.get("n_rows", 0), klt_use_prior=sp.get("use_prior", True)))
    return steps


def _tracker(ctx, cal):
    t = ov2slam_amd.LockstepTracker(ctx, BATCH, W, H, use_clahe=False, nbmaxkps=N_MAX)
    t.setCalibration(cal)
    return t


def _first(t, how):
    z2, z3, z1 = np.zeros((BATCH, N_MAX, 2), np.float32), np.zeros((BATCH, N_MAX, 3)), np.zeros((BATCH, N_MAX), np.uint8)
    first = [_seqs()[b][0][0] for b in range(BATCH)]
    zn = np.zeros(BATCH, np.int32)
    if how == "route":
        return t.trackFrameMap(first, z2, z3, z1, np.tile(I7, (BATCH, 1)), zn)
    return t.trackFramePose(first, z2, z3, z1, np.tile(I7, (BATCH, 1)), zn, _params(), np.tile(I7, (BATCH, 1)), np.array([0, 1, 0], np.uint8),
                            np.arange(BATCH, dtype=np.uint64))


def _call(t, s, how, ctx):
    a = (s["imgs"], s["kps"], s["wpt"], s["is3d"], s["Tcw"], s["n"])
    kw = dict(scale=s["scale"], dop3p=s["dop3p"], n_rows=s["n_rows"], klt_use_prior=s["klt_use_prior"])
    if how == "route":
        out, st, rule, poses, inputs = F.route(ctx, t, *a, s["params"], s["Twc"], s["p3p_req"], s["seed"], **kw)
    else:
        if how == "fused":
            out, st, rule, poses = t.trackFramePose(*a, s["params"], s["Twc"], s["p3p_req"], s["seed"], **kw)
        else:
            t.trackFramePoseBegin(*a, s["params"], s["Twc"], s["p3p_req"], s["seed"], **kw)
            out, st, rule, poses = t.trackFramePoseEnd()
        inputs = [t.lastPoseInputs(b) for b in range(len(s["imgs"]))]
    na = len(s["imgs"])
    kp = [t.lastKeypoints(b, int(s["n"][b])) for b in range(na)]
    pr = [t.lastPriors(b, int(s["n"][b])) for b in range(na)]
    return dict(out=out, st=st, rule=rule, poses=poses, inputs=inputs, kp=kp, pr=pr)


def _play(ctx, name, how, camera=None):
    """the sequence `name` on a fresh tracker, through route() ('route'), the one-call fused step ('fused') or its two halves
    ('halves'), under the EuRoC calibration or a camera of tests/camera_cases.py.  Computed once per (name, how, camera) and shared
    between the tests; nobody changes a result."""
    key = (name, how) if camera is None else (name, how, camera)
    if key not in _RUNS:
        cal = CC.calibration(ctx, camera) if camera else ov2slam_amd.CameraCalibration(ctx, "pinhole", *K, D=DIST)
        t = _tracker(ctx, cal)
        _first(t, "route" if how == "route" else "fused")
        _RUNS[key] = [_call(t, s, how, ctx) for s in _inputs(name, cal)]
        t.close()
    return _RUNS[key]


def _same_step(a, b, where):
    assert np.array_equal(_bits(a["out"]), _bits(b["out"])), (where, "positions")
    assert np.array_equal(a["st"], b["st"]), (where, "status")
    assert np.array_equal(a["rule"], b["rule"]), (where, "p3p_req")
    for i, (x, y) in enumerate(zip(a["kp"], b["kp"])):
        assert np.array_equal(_bits(x[0]), _bits(y[0])) and np.array_equal(x[1].view(np.uint64), y[1].view(np.uint64)), (where, i, "lastKeypoints")
    for i, (x, y) in enumerate(zip(a["pr"], b["pr"])):
        assert np.array_equal(_bits(x[0]), _bits(y[0])) and np.array_equal(x[1], y[1]), (where, i, "lastPriors")
    assert len(a["poses"]) == len(b["poses"])
    for i, (x, y) in enumerate(zip(a["poses"], b["poses"])):
        bx, by = F.pose_bytes(x), F.pose_bytes(y)
        for k in bx:
            assert bx[k] == by[k], (where, "item %d" % i, k, x["action"], y["action"])
    for i, (x, y) in enumerate(zip(a["inputs"], b["inputs"])):
        assert x[0] == y[0] and np.array_equal(x[1], y[1]) and np.array_equal(x[2], y[2]), (where, i, "lastPoseInputs")


@pytest.mark.parametrize("name", sorted(SPECS))
def test_fused_step_equals_the_route(gpu_ctx, name):
    A, B = _play(gpu_ctx, name, "route"), _play(gpu_ctx, name, "fused")
    for f, (a, b) in enumerate(zip(A, B)):
        print(name, f, [(pose.ACTION_NAMES[p["action"]], i[0], p["ran_p3p"], p["n_removed_p3p"], p["n_outliers_pnp"], p["passes"][1]["ran"])
                        for p, i in zip(a["poses"], a["inputs"])], "rule", a["rule"].astype(int).tolist())
    for f, (a, b) in enumerate(zip(A, B)):
        _same_step(a, b, (name, f))


@pytest.mark.parametrize("camera", CC.ADDED_FOLD)
def test_fused_step_equals_the_route_under_added_cameras(gpu_ctx, oracle, camera):
    """The main sequence under the added cameras, and one step under fisheye_fold: fused against route byte for byte as above, and
    after every step every item is tied to the reference (camera_cases.assert_step_anchor): lastKeypoints equals the stand-alone
    call on the output positions as bits, that call equals the oracle within the camera's bound, and the priors derived on the
    device equal ov2_klt_priors_batch as bits."""
    name = "fold" if camera == "fisheye_fold" else "main"
    cal = CC.calibration(gpu_ctx, camera)
    steps = _inputs(name, cal)
    A, B = _play(gpu_ctx, name, "route", camera), _play(gpu_ctx, name, "fused", camera)
    assert len(A) == len(B) == len(steps)
    for f, (s, a, b) in enumerate(zip(steps, A, B)):
        _same_step(a, b, (camera, name, f))
        CC.assert_step_anchor(gpu_ctx, oracle, cal, camera, s, b)
    if camera == "fisheye_fold":
        # the pose sets of both items hold failed and successful undistortions, the search and both passes ran on them
        for bi in (0, 1):
            m, slots, tab = B[0]["inputs"][bi]
            kind = CC.fisheye_kinds(camera, B[0]["out"][bi][slots])
            assert (kind != CC.OK).sum() >= 5 and (kind == CC.OK).sum() >= 5, (bi, CC.population(camera, B[0]["out"][bi][slots]))
            p = B[0]["poses"][bi]
            assert p["ran_p3p"] and len(tab) == 40
    else:
        assert [p["action"] for p in A[0]["poses"]] == [pose.POSE_OK, pose.POSE_OK, pose.TOO_FEW]
        assert A[2]["rule"].tolist() == [False, True, True]


def test_the_route_exercises_what_the_cases_are_for(gpu_ctx):
    """on the route's side alone: the sequences reach the branches they were built for"""
    A, Z = _play(gpu_ctx, "main", "route"), _play(gpu_ctx, "alt", "route")
    # counts and the 3-D share: 64 / 37 / 0 keypoints, a pose from the larger two
    assert [p["action"] for p in A[0]["poses"]] == [pose.POSE_OK, pose.POSE_OK, pose.TOO_FEW]
    assert 30 < A[0]["inputs"][0][0] < 64 and A[0]["inputs"][2][0] == 0
    # wrong map points: pass 2 ran and removed == 2 exists
    assert any(p["n_outliers_pnp"] > 0 and p["passes"][1]["ran"] for p in A[1]["poses"])
    assert any((p["removed"] == 2).any() for p in A[1]["poses"])
    # wrong motion model: the rule fires on every item with keypoints, the search runs there
    assert A[2]["rule"].tolist() == [False, True, True] and (A[2]["st"] & 2).any()
    assert all(p["ran_p3p"] for p in A[2]["poses"][1:]) and not A[2]["poses"][0]["ran_p3p"]
    # p3p_req on two items while the third has ended
    assert len(A[3]["poses"]) == 2 and all(p["ran_p3p"] for p in A[3]["poses"]) and not A[3]["rule"].any()
    # dop3p on all, both modes
    for f in (0, 1):
        ran = [p["ran_p3p"] for p in Z[f]["poses"]]
        assert ran == [i[0] >= 4 for i in Z[f]["inputs"]] and sum(ran) == 2, (f, ran)
        assert all(len(i[2]) == (40 if i[0] >= 4 else 0) for i in Z[f]["inputs"])
    # exactly 3, 4 and 5 3-D slots, all tracked: TOO_FEW, and two searches
    assert [i[0] for i in Z[2]["inputs"]] == [3, 4, 5]
    assert Z[2]["poses"][0]["action"] == pose.TOO_FEW and not Z[2]["poses"][0]["ran_p3p"]
    assert Z[2]["poses"][1]["ran_p3p"] and Z[2]["poses"][2]["ran_p3p"]
    # removed speaks of slots: nothing outside the pose set is ever marked
    for run in (A, Z):
        for s in run:
            for p, i in zip(s["poses"], s["inputs"]):
                outside = np.ones(len(p["removed"]), bool); outside[i[1]] = False
                assert not p["removed"][outside].any()


def test_the_device_draw_is_the_host_draw(gpu_ctx):
    """lastPoseInputs of the fused step against pose_set and ov2_p3p_draw_samples directly (not through the route)"""
    cal = ov2slam_amd.CameraCalibration(gpu_ctx, "pinhole", *K, D=DIST)
    seen = 0
    for name in sorted(SPECS):
        steps, B = _inputs(name, cal), _play(gpu_ctx, name, "fused")
        for f, (s, r) in enumerate(zip(steps, B)):
            for b, (m, slots, tab) in enumerate(r["inputs"]):
                want = F.pose_set(r["st"][b], s["is3d"][b], int(s["n"][b]))
                assert m == len(want) and np.array_equal(slots, want), (name, f, b)
                search = (s["p3p_req"][b] or r["rule"][b] or s["dop3p"]) and m >= 4
                assert np.array_equal(tab, pose.draw_samples(int(s["seed"][b]), m, s["n_rows"]) if search else np.zeros((0, 4), np.int32)), (name, f, b)
                seen += len(tab) > 0
    assert seen >= 8


def test_begin_end_equals_the_one_call_form(gpu_ctx):
    for f, (a, b) in enumerate(zip(_play(gpu_ctx, "main", "fused"), _play(gpu_ctx, "main", "halves"))):
        _same_step(a, b, ("halves", f))


def test_a_second_run_on_fresh_trackers_gives_the_same_bytes(gpu_ctx):
    first = _play(gpu_ctx, "main", "fused")
    del _RUNS[("main", "fused")]
    try:
        again = _play(gpu_ctx, "main", "fused")
    finally:
        _RUNS[("main", "fused")] = first
    for f, (a, b) in enumerate(zip(first, again)):
        _same_step(a, b, ("repeat", f))


def test_first_frame_and_empty_step_run_nothing(gpu_ctx):
    cal = ov2slam_amd.CameraCalibration(gpu_ctx, "pinhole", *K, D=DIST)
    t = _tracker(gpu_ctx, cal)
    Twc = np.stack([_rand_pose(np.random.default_rng(b)) for b in range(BATCH)])
    req = np.array([0, 1, 0], np.uint8)
    z2, z3, z1 = np.zeros((BATCH, N_MAX, 2), np.float32), np.zeros((BATCH, N_MAX, 3)), np.zeros((BATCH, N_MAX), np.uint8)
    seqs = _seqs()
    for f, n in enumerate(([5, 0, 9], [0, 0, 0])):                # the first frame (with keypoints passed), then a step that tracks nothing
        out, st, rule, poses = t.trackFramePose([seqs[b][0][f] for b in range(BATCH)], z2 + 50, z3 + 1, z1 + 1, np.tile(I7, (BATCH, 1)), n,
                                                _params(), Twc, req, np.arange(BATCH, dtype=np.uint64), dop3p=True, n_rows=10)
        assert not st.any() and not rule.any()
        for b in range(BATCH):
            want, got = F.pose_bytes(F.nothing_ran(Twc[b], req[b], n[b])), F.pose_bytes(poses[b])
            assert want == got, (f, b)
            assert t.lastPoseInputs(b)[0] == 0 and len(t.lastPoseInputs(b)[2]) == 0
    t.close()


def test_rejected_calls_leave_outputs_and_tracker_untouched(gpu_ctx):
    """every refusal is OV2_EINVAL before anything is enqueued; the next valid step equals tracker A's; a step begun with the pose
    form and finished with the plain end call gives the tracking half and drops the pose"""
    import ctypes as C
    cal = ov2slam_amd.CameraCalibration(gpu_ctx, "pinhole", *K, D=DIST)
    steps, A = _inputs("main", cal), _play(gpu_ctx, "main", "route")
    s = steps[0]
    a = (s["imgs"], s["kps"], s["wpt"], s["is3d"], s["Tcw"], s["n"])
    t = ov2slam_amd.LockstepTracker(gpu_ctx, BATCH, W, H, use_clahe=False, nbmaxkps=N_MAX)
    with pytest.raises(ov2slam_amd.Ov2Error) as e:                # no calibration
        t.trackFramePose(*a, s["params"], s["Twc"], s["p3p_req"], s["seed"])
    assert e.value.code == L.OV2_EINVAL and "calibration" in str(e.value)
    t.setCalibration(cal)
    _first(t, "fused")
    nan_wpt = s["wpt"].copy()
    nan_wpt[1, np.nonzero(s["is3d"][1])[0][0], 2] = np.nan
    sc61 = np.zeros((BATCH, N_MAX), np.int32); sc61[0, 3] = 61
    bad = [dict(n_rows=L.OV2_P3P_MAX_ROWS + 1), dict(scale=sc61), dict(wpt=nan_wpt), dict(n_rows=-1),
           dict(Twc=np.where(np.arange(7) == 2, np.inf, s["Twc"])), dict(chi2th=-1.0)]
    for kw in bad:
        prm = dict(s["params"], pnp=dict(s["params"]["pnp"], chi2th=kw["chi2th"])) if "chi2th" in kw else s["params"]
        with pytest.raises(ov2slam_amd.Ov2Error) as e:
            t.trackFramePose(s["imgs"], s["kps"], kw.get("wpt", s["wpt"]), s["is3d"], s["Tcw"], s["n"], prm, kw.get("Twc", s["Twc"]),
                             s["p3p_req"], s["seed"], scale=kw.get("scale"), n_rows=kw.get("n_rows", 0))
        assert e.value.code == L.OV2_EINVAL, kw.keys()
    # NULL Twc_h through the C ABI, with poisoned outputs: nothing is written
    c = t._marshal_track_frame_pose(*a, s["params"], s["Twc"], s["p3p_req"], s["seed"])
    c.inputs.Twc_h = None
    na = c.na
    out = np.full((BATCH, N_MAX, 2), 7.5, np.float32); st = np.full((BATCH, N_MAX), 0x6E, np.uint8); p3p = np.full(na, 0x6E6E, np.int32)
    res = lockstep._Results(t, "track_frame_pose", c)
    R, removed = res.R, res.removed
    removed[...] = 0x6E
    before = bytes(C.string_at(C.byref(R), C.sizeof(R)))
    rc = t.lib.ov2_btracker_track_frame_pose(t.h_trk, *c.args, out.ctypes.data, st.ctypes.data, p3p.ctypes.data, R)
    assert rc == L.OV2_EINVAL and b"NULL" in t.lib.ov2_last_error()
    assert (out == 7.5).all() and (st == 0x6E).all() and (p3p == 0x6E6E).all() and (removed == 0x6E).all()
    assert bytes(C.string_at(C.byref(R), C.sizeof(R))) == before
    # the tracker is where it was: the same frames pass now, and give what tracker A gave
    got = _call(t, s, "fused", gpu_ctx)
    _same_step(A[0], got, "after the refusals")
    # the pose form finished by the plain end call: the tracking half, no pose
    s1 = steps[1]
    t.trackFramePoseBegin(s1["imgs"], s1["kps"], s1["wpt"], s1["is3d"], s1["Tcw"], s1["n"], s1["params"], s1["Twc"], s1["p3p_req"], s1["seed"],
                          klt_use_prior=s1["klt_use_prior"])
    out, st, rule = t.trackFrameEnd()
    assert np.array_equal(_bits(out), _bits(A[1]["out"])) and np.array_equal(st, A[1]["st"]) and np.array_equal(rule, A[1]["rule"])
    got = _call(t, steps[2], "fused", gpu_ctx)
    _same_step(A[2], got, "after the plain end call")
    t.close()
