"""ov2_btracker_mono_init (scope row f25; csrc/trackb_monoinit.hip, csrc/monoinit.hip) against the cycle of separate calls it replaces
(tests/monoinit_ref.py: route).  Two trackers play the same mono start -- a first frame, createKeyframe, then trackMonoResident
steps on shifted images, each followed by the initialisation test with do = [1, 1, 1, 0] --, tracker A through the route, tracker B
through the new call, whole or as _begin / _end.  EVERY comparison is on raw bytes: both sides run the same device code on the same
inputs, so equality is the requirement, not a tolerance.  Compared after every call: every field of every record and the removal
bytes, the resident frame (B's device block and B's host mirror against A's), the resident pose and the motion state; then every
field of one more trackMonoResident step played on both, which is what exposes a motion state that was not reset.

Shapes: 376 x 240 without distortion (pinhole) and 161 x 121 with it (fisheye), batch 4, 200 slots, about a hundred keypoints a frame.
Item 0 moves 4 px a frame and is READY at the second step (finit_parallax is 6 px), where seven of its keypoints have been moved off
their tracks and leave the frame as the search's outliers; item 1 stands still (LOW_PARALLAX), item 2 moves
but keeps 40 keypoints (RESET, min_2d_kps = 50), item 3 moves and is not asked."""
import numpy as np
import pytest

import ov2slam_amd
from ov2slam_amd import _lib as L
from ov2slam_amd import Ov2Error, pose
from tests import fivept_ref as E5
from tests import kfreq_ref as KF
from tests import monoinit_ref as R
from tests import resident_ref as RR
from tests import stereokf_ref as SR
from tests import temporalkf_ref as TR
from tests.test_gpu_framepose import _params
from tests.test_gpu_trackmono import _same_mono_step

pytestmark = pytest.mark.gpu

N_MAX, FINIT, POISON = 200, 6.0, 0x5A
CELLS = {"mono-pinhole": 30, "stereo-fisheye": 14}                        # 13 x 8 and 12 x 9 detection cells
DO = [1, 1, 1, 0]
_RUNS = {}


def _images(cfg, f):
    """frame f of every item: a crop of the item's texture moved 4 px right and 1 px down a frame; item 1 stands still"""
    return [SR.pair(cfg, b, (0, 0) if b == 1 else (4 * f, f))[0] for b in range(cfg["batch"])]


def _P(cfg, Kc, cell, n_rows=64):
    fkf = KF.make_params(K=Kc, img_w=cfg["w"], img_h=cfg["h"], ncellsize=cell, stereo=False, nbmaxkps=N_MAX, finit_parallax=FINIT)
    return dict(fkf=fkf, max_iterations=100, threshold=E5.threshold_of(3.0, Kc[0], Kc[1]), probability=0.99, n_rows=n_rows, min_2d_kps=50)


def _step_args(cfg, P, Kc, f):
    B = cfg["batch"]
    epi = dict(fkf=P["fkf"], max_iterations=100, threshold=P["threshold"], probability=0.99, fransac_err=3.0, mono=True, n_rows=48)
    seeds = lambda k: (np.arange(B, dtype=np.uint64) + np.uint64(k)) * np.uint64(2) + np.uint64(1)
    return (_params(pose.LMEDS, False, Kc), epi, np.zeros(B, np.uint8), seeds(10 * f), np.full(B, 1, np.int32), seeds(10 * f + 5),
            np.full(B, 10.0 + 0.05 * f), np.arange(B, dtype=np.int32) + f)


class _Side:
    def __init__(self, ctx, name, which, how):
        self.ctx, self.which, self.how = ctx, which, how
        cfg = self.cfg = TR.CONFIGS[name]
        self.B, self.cell = cfg["batch"], CELLS[name]
        K, _ = TR.camera(cfg)
        self.Kc = tuple(float(v) for v in K)
        self.cal = ov2slam_amd.CameraCalibration(ctx, cfg["model"], *K, D=cfg["D"])
        self.t = ov2slam_amd.LockstepTracker(ctx, self.B, cfg["w"], cfg["h"], use_clahe=False, nbmaxkps=N_MAX)
        self.t.setCalibration(self.cal)
        self.P = _P(cfg, self.Kc, self.cell)
        self.kf = [None] * self.B
        self.log = []

    def views(self):
        t, B = self.t, self.B
        return dict(device=[RR.frame_bytes(t.getFrame(b, True)) for b in range(B)], mirror=[RR.frame_bytes(t.getFrame(b, False)) for b in range(B)],
                    res_T=np.array([t.getPose(b) for b in range(B)]).tobytes(), res_s=[t.getMotion(b) for b in range(B)])

    def note(self, kind, **kw):
        self.log.append(dict(kind=kind, views=self.views(), **kw))
        return self.log[-1]

    def step(self, f, tag):
        t, B = self.t, self.B
        nb = [t.getFrame(b, False)["n"] for b in range(B)]
        out, st, rule, epis, poses, monos, frames = t.trackMonoResident(_images(self.cfg, f), *_step_args(self.cfg, self.P, self.Kc, f))
        nk = [0] * B if f == 0 else nb                                    # the tracker's first frame tracks nothing
        return self.note(tag, nb=nb, out=out, st=st, rule=rule, epis=epis, poses=poses, monos=monos, frames=frames,
                         res_T=np.array([t.getPose(b) for b in range(B)]), res_s=[t.getMotion(b) for b in range(B)],
                         kp=[t.lastKeypoints(b, nk[b]) for b in range(B)], pr=[t.lastPriors(b, nk[b]) for b in range(B)],
                         inputs=[t.lastPoseInputs(b) for b in range(B)], einputs=[t.lastEpiInputs(b) for b in range(B)],
                         slot_bytes=t.lastSlotBytes())

    def ckf(self, tag):
        cfg, B, c = self.cfg, self.B, self.cell
        params = dict(ncellsize=c, nbwcells=int(np.ceil(cfg["w"] / c)), nbhcells=int(np.ceil(cfg["h"] / c)), nbmaxkps=N_MAX, detector="singlescale",
                      det_cell=c, roi=(5, 5, cfg["w"] - 10, cfg["h"] - 10), mask_mode=0, do_subpix=True, use_brief=False)
        ids = (100 + np.arange(B)).astype(np.int32)
        recs, o = self.t.createKeyframe(B, None, None, None, None, np.ones(B, np.uint8), np.zeros(B, np.int32), ids, np.full(B, 10.01), params,
                                        np.full(B, 1e-3, np.float64))
        for b, r in enumerate(recs):
            assert r["action"] == L.OV2_CKF_CREATED and r["n_new"] >= 60, r
            n = r["n_kf"]
            order = np.argsort(o["lmid"][b, :n], kind="stable")
            self.kf[b] = dict(Twc=self.t.getPose(b), lmid=o["lmid"][b, :n][order].copy(), unpx=o["unpx"][b, :n][order].copy(),
                              bv=o["bv"][b, :n][order].copy())
        return self.note(tag, ckf=recs)

    def thin(self, b, keep, tag):
        """the map drops all but `keep` keypoints of item b's frame (the same call on both sides)"""
        fr = self.t.getFrame(b, False)
        ops = [[] for _ in range(self.B)]
        ops[b] = [(int(v), L.OV2_RES_REMOVE, None) for v in fr["lmid"][keep:fr["n"]]]
        return self.note(tag, upd=self.t.updateFrame(self.B, ops))

    def mismatch(self, b, k, tag):
        """k keypoints of item b's frame end up 15 px across the motion (setFrame in mid-sequence, the same ids; the same call on
        both sides): matches the 5-point search must find to be outliers"""
        fr = self.t.getFrame(b, False)
        n = fr["n"]
        px = fr["px"][:n].copy()
        sel = np.nonzero((px[:, 1] > 20) & (px[:, 1] < self.cfg["h"] - 40))[0][::max(1, n // (2 * k))][:k]
        px[sel, 1] += np.float32(15.0)
        self.t.setFrame(b, px, fr["lmid"][:n], fr["is3d"][:n], fr["wpt"][:n])
        return self.note(tag, moved=fr["lmid"][sel].tolist())

    def init(self, f, do, tag, kf=None, P=None):
        B, t, P = self.B, self.t, self.P if P is None else P
        seeds = ((np.arange(B, dtype=np.uint64) + np.uint64(31 * f)) * np.uint64(2) + np.uint64(1))
        removed = np.full((B, N_MAX), POISON, np.uint8)
        if self.which == "A":
            recs, removed = R.route(self.ctx, t, self.cal, len(do), do, seeds, P, self.kf if kf is None else kf, removed)
            slot_bytes = None
        else:
            if self.how == "one":
                recs, out = t.monoInit(len(do), do, seeds, P, out=dict(removed=removed))
            else:
                t.monoInitBegin(len(do), do, seeds, P)
                recs, out = t.monoInitEnd(out=dict(removed=removed))
            assert out["removed"] is removed
            slot_bytes = t.lastSlotBytes()
        return self.note(tag, do=list(do), recs=recs, removed=removed, slot_bytes=slot_bytes)


def _play(ctx, name, which, how="one"):
    """the start of a mono sequence on a fresh tracker: side 'A' (the route) or 'B' (the new call; how: 'one' call or two 'halves')
    -> the log, one entry per call.  Computed once per key and shared; nobody changes a result."""
    key = (name, which, how)
    if key in _RUNS:
        return _RUNS[key]
    s = _Side(ctx, name, which, how)
    s.step(0, "first_frame")
    s.init(0, DO, "init_no_keyframe")                                     # before createKeyframe: no item has a keyframe
    s.ckf("ckf")
    s.thin(2, 40, "thin")
    s.step(1, "step1")
    s.init(1, DO, "init1")
    s.step(2, "step2")
    s.mismatch(0, 7, "mismatch")
    s.init(2, DO, "init2")
    s.step(3, "step3")
    s.t.close()
    _RUNS[key] = s.log
    return s.log


def _bytes(v):
    return np.ascontiguousarray(v).tobytes()


def _same_record(a, b, where):
    assert set(a) == set(b) == set(R.REC_KEYS), where
    for k in R.REC_KEYS:
        assert _bytes(a[k]) == _bytes(b[k]) or (isinstance(a[k], int) and a[k] == b[k]), (where, k, a[k], b[k])


def _same_views(va, vb, w):
    """frame (device block and mirror), pose and motion state of two trackers, or of one at two times"""
    assert va["device"] == vb["device"] == vb["mirror"] == va["mirror"], w
    assert va["res_T"] == vb["res_T"], w
    for sa, sb in zip(va["res_s"], vb["res_s"]):
        assert sorted(sa) == sorted(sb) and all(_bytes(sa[k]) == _bytes(sb[k]) for k in sa), w


def _same_log(A, B, where):
    assert [e["kind"] for e in A] == [e["kind"] for e in B]
    for ea, eb in zip(A, B):
        w = (where, ea["kind"])
        _same_views(ea["views"], eb["views"], w)
        if "recs" in ea:
            for b, (ra, rb) in enumerate(zip(ea["recs"], eb["recs"])):
                _same_record(ra, rb, w + (b,))
            assert np.array_equal(ea["removed"], eb["removed"]), w
        if "monos" in ea:
            _same_mono_step(ea, eb, w)
            assert ea["frames"] == eb["frames"] and ea["nb"] == eb["nb"], w
        if eb.get("slot_bytes") is not None and eb["kind"].startswith("init"):
            assert eb["slot_bytes"] == 0, w


@pytest.mark.parametrize("name", sorted(TR.CONFIGS))
@pytest.mark.parametrize("how", ("one", "halves"))
def test_the_call_equals_the_route(gpu_ctx, name, how):
    A, B = _play(gpu_ctx, name, "A"), _play(gpu_ctx, name, "B", how)
    for e in B:
        if e["kind"].startswith("init"):
            print(name, how, e["kind"], [(R.ACTIONS.get(r["action"], r["action"]), r["nb2dkps"], float(r["p0"]), r["m"], float(r["p1"]),
                                         r["n_inliers"], r["n_removed"]) for r in e["recs"]])
    _same_log(A, B, (name, how))


@pytest.mark.parametrize("name", sorted(TR.CONFIGS))
def test_the_scenario_takes_the_branches_it_is_for(gpu_ctx, name):
    log = {e["kind"]: e for e in _play(gpu_ctx, name, "A")}
    act = lambda k: [r["action"] for r in log[k]["recs"]]
    assert act("init_no_keyframe") == [R.NO_KEYFRAME, R.NO_KEYFRAME, R.NO_KEYFRAME, R.NOT_REQUESTED]
    assert act("init1") == [R.LOW_PARALLAX, R.LOW_PARALLAX, R.RESET, R.NOT_REQUESTED]
    assert act("init2") == [R.READY, R.LOW_PARALLAX, R.RESET, R.NOT_REQUESTED]
    r0, r1 = log["init2"]["recs"][0], log["init1"]["recs"][0]
    assert 0.0 < float(r1["p0"]) <= FINIT < float(r0["p0"]) and float(r0["p1"]) >= FINIT and r0["nb2dkps"] >= 50 and r0["m"] >= 50
    assert 8 <= log["init2"]["recs"][2]["nb2dkps"] <= 40
    # READY: the removed slots left the frame, the pose is Twc_init; every other item's frame and pose stayed
    before, after = log["mismatch"]["views"], log["init2"]["views"]
    n0 = before["mirror"][0]["n"]
    assert after["mirror"][0]["n"] == n0 - r0["n_removed"] and r0["n_removed"] >= 1 and r0["n_inliers"] >= 50
    flags = log["init2"]["removed"][0]
    assert int((flags[:n0] == 1).sum()) == r0["n_removed"] and (flags[n0:] == POISON).all()
    # what stays is what was not flagged, in slot order; some of what left had been moved off its track
    ids = np.frombuffer(before["mirror"][0]["lmid"], np.int32)
    assert np.array_equal(np.frombuffer(after["mirror"][0]["lmid"], np.int32), ids[flags[:n0] == 0])
    assert set(ids[flags[:n0] == 1].tolist()) & set(log["mismatch"]["moved"]) and len(log["mismatch"]["moved"]) == 7
    assert np.frombuffer(after["res_T"], np.float64).reshape(4, 7)[0].tobytes() == r0["Twc_init"].tobytes()
    assert abs(np.linalg.norm(r0["Twc_init"][:3]) - 0.25) < 1e-15 and r0["pose_refined"] == 0
    for b in (1, 2, 3):
        assert after["mirror"][b] == before["mirror"][b] and after["device"][b] == before["device"][b]
        assert after["res_T"][56 * b:56 * b + 56] == before["res_T"][56 * b:56 * b + 56]
    # the motion state: reset for every item that ran, left alone for the one that was not asked
    for b in (0, 1, 2):
        s = after["res_s"][b]
        assert s["prev_time"] == -1.0 and not np.asarray(s["log_relT"]).any()
    assert after["res_s"][3]["prev_time"] == before["res_s"][3]["prev_time"] != -1.0
    assert _bytes(after["res_s"][3]["log_relT"]) == _bytes(before["res_s"][3]["log_relT"])
    # ... and untouched removal bytes for the items that did not run
    assert (log["init2"]["removed"][3] == POISON).all() and (log["init_no_keyframe"]["removed"] == POISON).all()


def test_refusals_leave_the_tracker_where_it_was(gpu_ctx):
    name = "mono-pinhole"
    s = _Side(gpu_ctx, name, "B", "one")
    t, B = s.t, s.B
    seeds = np.arange(B, dtype=np.uint64)
    with pytest.raises(Ov2Error):                                         # no resident frame yet
        t.monoInit(B, DO, seeds, s.P)
    s.step(0, "first_frame")
    s.ckf("ckf")
    s.step(1, "step1")
    v0 = s.views()
    bad = [dict(s.P, min_2d_kps=-1), dict(s.P, n_rows=-1), dict(s.P, n_rows=4097), dict(s.P, boptimize=True), dict(s.P, threshold=0.0),
           dict(s.P, probability=1.0), dict(s.P, max_iterations=-1), dict(s.P, fkf=dict(s.P["fkf"], finit_parallax=float("nan"))),
           dict(s.P, fkf=dict(s.P["fkf"], K=(1.0, 1.0, float("inf"), 0.0)))]
    for P in bad:
        with pytest.raises(Ov2Error) as e:
            t.monoInit(B, DO, seeds, P)
        assert e.value.code == L.OV2_EINVAL
    for na in (0, B + 1):
        with pytest.raises(Ov2Error):
            t.monoInit(na, [1] * (B + 1), np.arange(B + 1, dtype=np.uint64), s.P)
    with pytest.raises(Ov2Error):                                         # _end with nothing open
        t.monoInitEnd()
    _same_views(s.views(), v0, "after the refusals")
    # an open call: nothing that changes resident state or starts a step gets through, and a second _begin is refused
    t.monoInitBegin(B, DO, seeds, s.P)
    for call in (lambda: t.monoInitBegin(B, DO, seeds, s.P), lambda: t.setPose(0, np.array([0, 0, 0, 0, 0, 0, 1.0])), lambda: t.resetMotion(0),
                 lambda: t.updateFrame(B, [[] for _ in range(B)]), lambda: t.setFrame(0, np.zeros((0, 2), np.float32), [], [], np.zeros((0, 3))),
                 lambda: t.trackMonoResidentBegin(_images(s.cfg, 2), *_step_args(s.cfg, s.P, s.Kc, 2)),
                 lambda: t.temporalKeyframeEnd(), lambda: t.createKeyframeEnd()):
        with pytest.raises(Ov2Error) as e:
            call()
        assert e.value.code == L.OV2_EINVAL
    recs, out = t.monoInitEnd()
    assert [r["action"] for r in recs] == [R.LOW_PARALLAX, R.LOW_PARALLAX, R.LOW_PARALLAX, R.NOT_REQUESTED] and t.lastSlotBytes() == 0
    # NULL arguments, through the ABI itself: params, do_h, seed_h, and the whole call's results / removed_h
    import ctypes as C
    from ov2slam_amd import keyframe
    from ov2slam_amd.frontend import _ptr
    v1 = s.views()
    p, do, rm = keyframe._as_mono_init_params(s.P), np.array(DO, np.uint8), np.zeros((B, N_MAX), np.uint8)
    res = (L.MonoInitResult * B)()
    good = (B, C.byref(p), _ptr(do), _ptr(seeds))
    for k in (1, 2, 3):
        a = list(good)
        a[k] = None
        assert t.lib.ov2_btracker_mono_init_begin(t.h_trk, *a) == L.OV2_EINVAL and b"NULL" in t.lib.ov2_last_error()
    assert t.lib.ov2_btracker_mono_init_begin(None, *good) == L.OV2_EINVAL
    assert t.lib.ov2_btracker_mono_init(t.h_trk, *good, None, _ptr(rm)) == L.OV2_EINVAL
    assert t.lib.ov2_btracker_mono_init(t.h_trk, *good, res, None) == L.OV2_EINVAL
    assert t.lib.ov2_btracker_mono_init_end(t.h_trk, res, _ptr(rm)) == L.OV2_EINVAL         # none of them opened a call
    _same_views(s.views(), v1, "after the NULL arguments")
    # a tracker without a calibration; the same tracker with one, but with no resident block
    t2 = ov2slam_amd.LockstepTracker(gpu_ctx, B, s.cfg["w"], s.cfg["h"], use_clahe=False, nbmaxkps=N_MAX)
    t2.setFrame(0, np.zeros((0, 2), np.float32), [], [], np.zeros((0, 3)))
    with pytest.raises(Ov2Error) as e:
        t2.monoInit(B, DO, seeds, s.P)
    assert e.value.code == L.OV2_EINVAL and "calibration" in str(e.value)
    t2.close()
    t3 = ov2slam_amd.LockstepTracker(gpu_ctx, B, s.cfg["w"], s.cfg["h"], use_clahe=False, nbmaxkps=N_MAX)
    t3.setCalibration(s.cal)
    with pytest.raises(Ov2Error) as e:
        t3.monoInit(B, DO, seeds, s.P)
    assert e.value.code == L.OV2_EINVAL and "resident frame" in str(e.value)
    t3.close()
    # a tracker whose frames may hold more keypoints than a chain takes
    t4 = ov2slam_amd.LockstepTracker(gpu_ctx, 1, 64, 48, use_clahe=False, nbmaxkps=L.OV2_FKF_MAX_POINTS + 1)
    t4.setCalibration(s.cal)
    with pytest.raises(Ov2Error) as e:
        t4.monoInit(1, [1], seeds[:1], s.P)
    assert e.value.code == L.OV2_EINVAL and "OV2_FKF_MAX_POINTS" in str(e.value)
    t4.close()
    t.close()
