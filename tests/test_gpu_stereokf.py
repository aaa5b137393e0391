"""ov2_btracker_stereo_keyframe (scope row f22; csrc/stereokf.hip, csrc/trackb_keyframe.hip): the mapper's stereo block on the resident keyframe
in one lock-step call, against the route of separate calls it replaces (tests/stereokf_ref.py: route).  Tracker A plays the scenario
through the route, tracker B through the new call; EVERY comparison is on raw bytes: both sides run the same device code on the same
inputs, so equality is the requirement, not a tolerance, and no point is left out.  Compared after every call: every field of every
record, the five per-slot outputs (scattered into poisoned arrays: what a call does not write stays poison on both sides), the frame
from the device and from the mirror, the keyframe info from both, lastSlotBytes() == 0 on B; and at the end a trackMonoResident step on
both trackers, whose kf.decision reads the new kf_nb3dkps and whose priors read the new points.

Shapes: 376 x 240 without CLAHE, batch 4, 160 slots, cell 35 for `rect` and `unrect-radtan`; 161 x 121, batch 2 for `unrect-fisheye`.
The frames are installed with setFrame and turned into keyframes by the resident createKeyframe, so that old slots and fresh
detections are both present.  What the frames make the block do is asserted without a GPU in tests/test_stereokf_reference.py; here
test_the_route_takes_every_branch asserts it on A's records."""
import numpy as np
import pytest

import ov2slam_amd
from ov2slam_amd import _lib as L
from ov2slam_amd import pose
from tests import fivept_ref as E5
from tests import kfreq_ref as KF
from tests import resident_ref as RR
from tests import stereokf_ref as R
from tests.test_gpu_framepose import _params
from tests.test_gpu_trackmono import _same_mono_step

pytestmark = pytest.mark.gpu

POISON = 0x5A
N_MAX, CELL = R.N_MAX, R.CELL
NOT_REQUESTED, NOT_KEYFRAME, DONE = L.OV2_SKF_NOT_REQUESTED, L.OV2_SKF_NOT_KEYFRAME, L.OV2_SKF_DONE
SIZES = (0, 1, 64, 65)                                                   # and 160 on item 0 afterwards
SIZE_P3D = {0: 0.35, 1: 1.0, 64: 1.0, 65: 0.0, 160: 0.35}               # 64: every slot 3-D; 65: none
_RUNS = {}


def _grid(cfg):
    return int(np.ceil(cfg["w"] / CELL)), int(np.ceil(cfg["h"] / CELL))


def _step_args(S, f):
    cfg, Kc, B = S["cfg"], tuple(float(v) for v in S["K"]), S["cfg"]["batch"]
    nbw, nbh = _grid(cfg)
    fkf = KF.make_params(K=Kc, img_w=cfg["w"], img_h=cfg["h"], stereo=True, nbmaxkps=nbw * nbh)
    epi = dict(fkf=fkf, max_iterations=100, threshold=E5.threshold_of(3.0, Kc[0], Kc[1]), probability=0.99, fransac_err=3.0, mono=False, n_rows=48)
    seeds = lambda k: (np.arange(B, dtype=np.uint64) + np.uint64(k)) * np.uint64(2) + np.uint64(1)
    return (_params(pose.LMEDS, False, Kc), epi, np.zeros(B, np.uint8), seeds(10 * f), np.full(B, 3, np.int32), seeds(10 * f + 5),
            np.full(B, 10.0 + 0.05 * f), np.arange(B, dtype=np.int32) + f)


def _ckf_params(cfg, nbmaxkps):
    nbw, nbh = _grid(cfg)
    return dict(ncellsize=CELL, nbwcells=nbw, nbhcells=nbh, nbmaxkps=nbmaxkps, detector="singlescale", det_cell=CELL,
                roi=(5, 5, cfg["w"] - 10, cfg["h"] - 10), mask_mode=0, do_subpix=True, use_brief=False)


class _Side:
    """one tracker and the bookkeeping of the scenario: which items' frames are their keyframes, the map's id counters, the keyframes"""

    def __init__(self, ctx, name, which, how):
        self.ctx, self.S, self.which, self.how = ctx, R.scenario(name), which, how
        cfg = self.cfg = self.S["cfg"]
        self.B = cfg["batch"]
        self.t = ov2slam_amd.LockstepTracker(ctx, self.B, cfg["w"], cfg["h"], use_clahe=False, nbmaxkps=N_MAX)
        self.t.setCalibration(R.calibrations(ctx, self.S)[0])
        self.skp = R.skf_params(ctx, self.S)
        self.rp = ov2slam_amd.Pyramid(ctx, cfg["w"], cfg["h"], R.WIN, 3, batch=self.B).build(np.stack([it["right"] for it in self.S["items"]]))
        self.iskf, self.nlmid = [False] * self.B, np.zeros(self.B, np.int32)
        self.kf = [dict(id=0, time=0.0, Twc=it["Twc"]) for it in self.S["items"]]
        self.state = np.full(self.B, 1e-3, np.float64)
        self.log = []

    def views(self):
        t = self.t
        return dict(device=[RR.frame_bytes(t.getFrame(b, True)) for b in range(self.B)],
                    mirror=[RR.frame_bytes(t.getFrame(b, False)) for b in range(self.B)],
                    info_device=[t.getKeyframeInfo(b, True) for b in range(self.B)], info_mirror=[t.getKeyframeInfo(b, False) for b in range(self.B)])

    def note(self, kind, **kw):
        self.log.append(dict(kind=kind, views=self.views(), **kw))
        return self.log[-1]

    def set_frame(self, b, f):
        self.t.setFrame(b, f["px"], f["lmid"], f["is3d"], f["wpt"])
        self.iskf[b] = False
        if f["n"]:
            self.nlmid[b] = max(int(self.nlmid[b]), int(np.max(f["lmid"])) + 1)

    def ckf(self, make_kf, nbmaxkps, round_, tag):
        mk = np.array(make_kf, np.uint8)
        ids = (100 * (round_ + 1) + np.arange(self.B)).astype(np.int32)
        times = np.full(self.B, 10.01 + round_)
        recs, _ = self.t.createKeyframe(len(mk), None, None, None, None, mk, self.nlmid.copy(), ids, times, _ckf_params(self.cfg, nbmaxkps),
                                        self.state)
        for b, r in enumerate(recs):
            if r["action"] == L.OV2_CKF_CREATED:
                self.nlmid[b] += r["n_new"]
                self.iskf[b] = True
                self.kf[b] = dict(id=int(ids[b]), time=float(times[b]), Twc=self.t.getPose(b))
        return self.note(tag, ckf=recs)

    def skf(self, do, tag):
        na = len(do)
        actions = [NOT_REQUESTED if not do[b] else (DONE if self.iskf[b] else NOT_KEYFRAME) for b in range(na)]
        out = R.empty_out(self.B, N_MAX, POISON)
        if self.which == "A":
            recs, out = R.route(self.ctx, self.t, self.rp, na, actions, self.S, self.kf, out)
            slot_bytes = None
        else:
            if self.how == "one":
                recs, out = self.t.stereoKeyframe(na, self.rp, do, self.skp, out=out)
            else:
                self.t.stereoKeyframeBegin(na, self.rp, do, self.skp)
                recs, out = self.t.stereoKeyframeEnd(out=out)
            slot_bytes = self.t.lastSlotBytes()
        assert [r["action"] for r in recs] == actions, (tag, recs, actions)
        return self.note(tag, do=list(do), recs=recs, out=out, slot_bytes=slot_bytes)

    def step(self, imgs, f, tag):
        t, B = self.t, self.B
        nb = [t.getFrame(b, False)["n"] for b in range(B)]
        out, st, rule, epis, poses, monos, frames = t.trackMonoResident(imgs, *_step_args(self.S, f))
        nk = [0] * B if f == 0 else nb                                    # the tracker's first frame tracks nothing
        rec = dict(out=out, st=st, rule=rule, epis=epis, poses=poses, monos=monos, frames=frames,
                   res_T=np.array([t.getPose(b) for b in range(B)]), res_s=[t.getMotion(b) for b in range(B)],
                   kp=[t.lastKeypoints(b, nk[b]) for b in range(B)], pr=[t.lastPriors(b, nk[b]) for b in range(B)],
                   inputs=[t.lastPoseInputs(b) for b in range(B)], einputs=[t.lastEpiInputs(b) for b in range(B)])
        return self.note(tag, nb=nb, **rec)


def _play(ctx, name, which, how="one"):
    """the scenario on a fresh tracker: side 'A' (the route) or 'B' (the new call; how: 'one' call or two 'halves') -> the log, one entry
    per call.  Computed once per key and shared; nobody changes a result."""
    key = (name, which, how)
    if key in _RUNS:
        return _RUNS[key]
    s = _Side(ctx, name, which, how)
    S, cfg, B, t = s.S, s.cfg, s.B, s.t
    items = S["items"]
    for b in range(B):
        t.setPose(b, items[b]["Twc"])
        s.set_frame(b, items[b]["frame"])
    s.step([it["left"] for it in items], 0, "first_frame")                # the tracker's first frame: the frames stay
    # the frames become keyframes, the detector tops them up; the stereo block for all but the last item of four
    nbw, nbh = _grid(cfg)
    s.ckf([1] * B, nbw * nbh, 0, "ckf_main")
    s.skf([1, 1, 1, 0] if B == 4 else [1] * B, "main")
    # item 1's frame is installed again (the same slots): it is no longer the keyframe's.  Everybody is asked: item 0 a second time (its
    # new 3-D points match and are not triangulated again), the last item for the first time
    f1 = t.getFrame(1, False)
    s.set_frame(1, f1)
    s.note("set_frame_again")
    s.skf([1] * B, "again")
    if B == 4:
        s.skf([0, 1, 1], "three_of_four")                                # n_active 3: item 3 is not looked at
    # frames of 0, 1, 64 and 65 slots (64: every slot 3-D, 65: none), keyframes without a top-up; then 160 slots
    for b, n in enumerate(SIZES[:B]):
        s.set_frame(b, R.make_frame(cfg, S["K"], S["iK"], items[b]["Twc"], n - n // 3, n // 3, int(s.nlmid[b]), 70 + b, p3d=SIZE_P3D[n]))
    s.ckf([1] * B, 0, 1, "ckf_sizes")
    s.skf([1] * B, "sizes")
    if B == 4:
        s.set_frame(0, R.make_frame(cfg, S["K"], S["iK"], items[0]["Twc"], 100, 60, int(s.nlmid[0]), 75, p3d=SIZE_P3D[160]))
        s.ckf([1, 0, 0, 0], 0, 2, "ckf_160")
        s.skf([1, 0, 0, 0], "size_160")
    # the step after: its priors read the new points, its keyframe decision the new kf_nb3dkps
    s.step([it["left2"] for it in items], 1, "step_after")
    t.close()
    s.rp.close()
    _RUNS[key] = s.log
    return s.log


def _same_log(A, B, where, route=True):
    assert [e["kind"] for e in A] == [e["kind"] for e in B]
    for i, (a, b) in enumerate(zip(A, B)):
        at = (where, i, a["kind"])
        if "monos" in a:
            _same_mono_step(a, b, at)
            assert a["frames"] == b["frames"] and a["nb"] == b["nb"], (at, a["frames"], b["frames"])
        elif "out" in a:
            assert a["recs"] == b["recs"], (at, a["recs"], b["recs"])
            for k in a["out"]:
                assert a["out"][k].tobytes() == b["out"][k].tobytes(), (at, k)
            assert b["slot_bytes"] == (0 if route else a["slot_bytes"]), (at, b["slot_bytes"])
        elif "ckf" in a:
            assert a["ckf"] == b["ckf"], (at, a["ckf"], b["ckf"])
        # both sides keep resident frames: A's device block, A's mirror, B's device block and B's mirror hold the same bytes
        for view in ("device", "mirror"):
            for item, (x, y) in enumerate(zip(a["views"]["device"], b["views"][view])):
                for k in x:
                    assert x[k] == y[k], (at, "frame of item %d" % item, view, k, x["n"], y["n"])
            assert a["views"]["device"] == a["views"]["mirror"], (at, "A's own mirror")
        for view in ("info_device", "info_mirror"):
            assert a["views"]["info_device"] == b["views"][view] == a["views"]["info_mirror"], (at, view, a["views"]["info_device"], b["views"][view])


def _show(name, A):
    for e in A:
        if "monos" in e:
            print(name, e["kind"], "frames", [(f["n_before"], f["n_after"]) for f in e["frames"]],
                  "kf", [(m["kf"]["n"], m["kf"]["nb3dkps"], m["kf"]["decision"], m["kf"]["reason"]) for m in e["monos"]])
        elif "out" in e:
            print(name, e["kind"], e["do"], [tuple(r[k] for k in R.REC_KEYS) for r in e["recs"]])
        elif "ckf" in e:
            print(name, e["kind"], [(r["action"], r["n_prev"], r["n_new"], r["n_kf"], r["nb3dkps"]) for r in e["ckf"]])


@pytest.mark.parametrize("how", ["one", "halves"])
@pytest.mark.parametrize("name", sorted(R.CONFIGS))
def test_the_call_equals_the_route_twice(gpu_ctx, name, how):
    """B against A after every call, and a second run of B on a fresh tracker against the first"""
    A, B = _play(gpu_ctx, name, "A"), _play(gpu_ctx, name, "B", how)
    _show(name, A)
    _same_log(A, B, (name, how))
    del _RUNS[(name, "B", how)]
    try:
        again = _play(gpu_ctx, name, "B", how)
    finally:
        _RUNS[(name, "B", how)] = B
    _same_log(A, again, (name, how, "repeat"))
    _same_log(B, again, (name, how, "B twice"), route=False)


@pytest.mark.parametrize("name", sorted(R.CONFIGS))
def test_the_route_takes_every_branch(gpu_ctx, name):
    """on A's side alone: the scenario reaches what it was built for"""
    A = _play(gpu_ctx, name, "A")
    _show(name, A)
    cfg = R.CONFIGS[name]
    B = cfg["batch"]
    by = {e["kind"]: e for e in A}
    # old slots and fresh detections: every item's keyframe holds more than setFrame installed
    assert all(r["action"] == L.OV2_CKF_CREATED and r["n_prev"] == cfg["n_inner"] + cfg["n_edge"] for r in by["ckf_main"]["ckf"])
    assert B < 4 or all(r["n_new"] > 0 for r in by["ckf_main"]["ckf"])
    main, again = by["main"], by["again"]
    recs = main["recs"]
    done = [b for b in range(B) if recs[b]["action"] == DONE]
    tot = {k: sum(recs[b][k] for b in done) for k in R.REC_KEYS}
    assert tot["n_prior3d"] >= 10 and (tot["n_prior_nb"] >= 10) == (not cfg["rect"])
    assert tot["n_stereo_kps"] > tot["n_stereo"] > tot["n_stereo_good"] >= 5      # matched 3-D keypoints are not tried; some are refused
    for b in done:
        n = recs[b]["n"]
        st, ok = main["out"]["tri_status"][b, :n], main["out"]["stereo_ok"][b, :n]
        before = np.frombuffer(by["ckf_main"]["views"]["device"][b]["is3d"], np.uint8)
        after = np.frombuffer(main["views"]["device"][b]["is3d"], np.uint8)
        good = (st & L.OV2_TRI_STEREO_OK) != 0
        assert np.array_equal(after, before | good) and recs[b]["nb3dkps"] == int(after.sum()) == main["views"]["info_device"][b]["kf_nb3dkps"]
        assert np.array_equal((st & L.OV2_TRI_STEREO_TRIED) != 0, (ok != 0) & (before == 0))
        assert not main["out"]["wpt"][b, :n][~good].any() and np.isfinite(main["out"]["wpt"][b, :n]).all()
        assert (main["out"]["right_px"][b, :n][ok != 0] != 0).any(axis=1).all()
    assert recs[1]["n_stereo"] > 0 and recs[1]["n_stereo_good"] <= recs[1]["n_stereo"] // 4      # the reversed pair: true matches are refused
    if B == 4:
        # the item that was not asked: its frame, its info and its output slots are what they were (poison)
        assert recs[3] == dict(dict.fromkeys(R.REC_KEYS, 0), action=NOT_REQUESTED)
        assert all((main["out"][k][3].view(np.uint8) == POISON).all() for k in main["out"])
        for view in ("device", "mirror", "info_device", "info_mirror"):
            assert main["views"][view][3] == by["ckf_main"]["views"][view][3]
        assert recs[2]["n_prior3d"] == 0 and recs[2]["n_stereo_kps"] == recs[2]["n_stereo"]      # an item without a 3-D slot
    # beyond n nothing is written
    for b in done:
        assert all((main["out"][k][b, recs[b]["n"]:].view(np.uint8) == POISON).all() for k in main["out"])
    # a frame changed by setFrame after its keyframe: NOT_KEYFRAME, nothing written
    r2 = again["recs"]
    assert r2[1] == dict(dict.fromkeys(R.REC_KEYS, 0), action=NOT_KEYFRAME)
    assert all((again["out"][k][1].view(np.uint8) == POISON).all() for k in again["out"])
    for view in ("device", "mirror", "info_device", "info_mirror"):
        assert again["views"][view][1] == by["set_frame_again"]["views"][view][1]
    # the second call on item 0: its new points are 3-D now, match again and are not triangulated again
    assert r2[0]["action"] == DONE and r2[0]["n_prior3d"] > recs[0]["n_prior3d"] and r2[0]["nb3dkps"] >= recs[0]["nb3dkps"]
    if B == 4:
        three = by["three_of_four"]
        assert len(three["recs"]) == 3 and [r["action"] for r in three["recs"]] == [NOT_REQUESTED, NOT_KEYFRAME, DONE]
        assert three["views"]["device"][3] == again["views"]["device"][3]
    # n of 0, 1, 64, 65 (and 160): every slot 3-D, and none
    sizes = by["sizes"]["recs"]
    assert [r["n"] for r in sizes] == list(SIZES[:B]) and all(r["action"] == DONE for r in sizes)
    if B == 4:
        assert sizes[2]["n_stereo"] == 0 and sizes[2]["nb3dkps"] == 64 and sizes[3]["n_prior3d"] == 0 and sizes[3]["n_stereo"] == sizes[3]["n_stereo_kps"]
        assert by["size_160"]["recs"][0]["n"] == 160 and by["size_160"]["recs"][0]["n_stereo_good"] > 0
    # the step after reads the new info
    step = by["step_after"]
    assert [m["kf"]["nb3dkps"] >= 0 for m in step["monos"]] and sum(f["n_before"] for f in step["frames"]) > 0


def test_refusals_leave_the_tracker_where_it_was(gpu_ctx):
    """every OV2_EINVAL / OV2_EUNSUPPORTED of the call returns before the tracker changes (the frame and the info are byte-equal before
    and after); while a call is open a second _begin, a step's _begin and the calls around the resident state are refused"""
    name = "unrect-radtan"
    s = _Side(gpu_ctx, name, "B", "one")
    S, cfg, B, t = s.S, s.cfg, s.B, s.t
    items = S["items"]

    def refused(call, words, code=L.OV2_EINVAL):
        with pytest.raises(ov2slam_amd.Ov2Error) as err:
            call()
        assert err.value.code == code and words in str(err.value), (words, str(err.value))

    do = [1] * B
    # no resident block yet, then no calibration, then no frame yet
    t2 = ov2slam_amd.LockstepTracker(gpu_ctx, B, cfg["w"], cfg["h"], use_clahe=False, nbmaxkps=N_MAX)
    refused(lambda: t2.stereoKeyframe(B, s.rp, do, s.skp), "no calibration")
    t2.setCalibration(R.calibrations(gpu_ctx, S)[0])
    refused(lambda: t2.stereoKeyframe(B, s.rp, do, s.skp), "no resident frame")
    f = items[0]["frame"]
    t2.setFrame(0, f["px"], f["lmid"], f["is3d"], f["wpt"])
    refused(lambda: t2.stereoKeyframe(B, s.rp, do, s.skp), "no current frames")
    t2.close()
    for b in range(B):
        t.setPose(b, items[b]["Twc"])
        s.set_frame(b, items[b]["frame"])
    s.step([it["left"] for it in items], 0, "first_frame")
    s.ckf([1] * B, 77, 0, "ckf_main")
    before = s.views()
    mk = lambda **kw: _changed(gpu_ctx, S, **kw)
    refused(lambda: t.stereoKeyframe(0, s.rp, do, s.skp), "n_active out of range")
    refused(lambda: t.stereoKeyframe(B + 1, s.rp, do + [1], s.skp), "n_active out of range")
    small = ov2slam_amd.Pyramid(gpu_ctx, cfg["w"], cfg["h"], R.WIN, 3, batch=B - 1)
    refused(lambda: t.stereoKeyframe(B, small, do, s.skp), "fewer items")
    for other in (ov2slam_amd.Pyramid(gpu_ctx, cfg["w"] - 8, cfg["h"], R.WIN, 3, batch=B), ov2slam_amd.Pyramid(gpu_ctx, cfg["w"], cfg["h"], 7, 3, batch=B),
                  ov2slam_amd.Pyramid(gpu_ctx, cfg["w"], cfg["h"], R.WIN, 2, batch=B)):
        refused(lambda: t.stereoKeyframe(B, other, do, s.skp), "differs from the tracker's")
        other.close()
    small.close()
    refused(lambda: t.stereoKeyframe(B, s.rp, do, mk(ncellsize=0)), "ncellsize not positive")
    refused(lambda: t.stereoKeyframe(B, s.rp, do, mk(tri_stereo=0)), "tri.stereo == 0")
    for field in ("Tcic0", "tri_Tcic0", "tri_Tlr"):
        refused(lambda: t.stereoKeyframe(B, s.rp, do, mk(**{field: np.nan})), "pose not finite")
    refused(lambda: t.stereoKeyframe(B, s.rp, do, mk(model=7)), "unknown camera model")
    refused(lambda: t.stereoKeyframe(B, s.rp, do, mk(nD=-1)), "bad distortion vector")
    refused(lambda: t.stereoKeyframe(B, s.rp, do, mk(nD=3)), "unsupported coefficient count", L.OV2_EUNSUPPORTED)
    refused(lambda: t.stereoKeyframe(B, s.rp, do, mk(img_w=0.0)), "img_w / img_h not positive")
    refused(lambda: t.stereoKeyframe(B, s.rp, do, mk(img_h=float("nan"))), "img_w / img_h not positive")
    refused(lambda: t.stereoKeyframe(B, s.rp, do, mk(nklt_win_size=7)), "not the pyramids' window")
    lib = t.lib
    R5 = (L.StereoKeyframeResult * B)()
    dob = (np.ones(B, np.uint8))
    assert lib.ov2_btracker_stereo_keyframe_begin(t.h_trk, B, None, s.rp.h_pyr, dob.ctypes.data) == L.OV2_EINVAL
    assert lib.ov2_btracker_stereo_keyframe_begin(t.h_trk, B, s.skp, None, dob.ctypes.data) == L.OV2_EINVAL
    assert lib.ov2_btracker_stereo_keyframe_begin(t.h_trk, B, s.skp, s.rp.h_pyr, None) == L.OV2_EINVAL
    assert lib.ov2_btracker_stereo_keyframe_end(t.h_trk, R5, None, None, None, None, None) == L.OV2_EINVAL
    assert b"without ov2_btracker_stereo_keyframe_begin" in lib.ov2_last_error()
    assert lib.ov2_btracker_stereo_keyframe(t.h_trk, B, s.skp, s.rp.h_pyr, dob.ctypes.data, None, None, None, None, None, None) == L.OV2_EINVAL
    assert s.views() == before and t.lastSlotBytes() == 0
    # an open step, an open createKeyframe call
    a1 = _step_args(S, 1)
    t.createKeyframeBegin(B, None, None, None, None, np.zeros(B, np.uint8), s.nlmid.copy(), np.arange(B, dtype=np.int32), np.full(B, 11.0),
                          _ckf_params(cfg, 0), s.state)
    refused(lambda: t.stereoKeyframe(B, s.rp, do, s.skp), "create_keyframe_begin has not been finished")
    t.createKeyframeEnd()
    assert s.views() == before
    # while a call of this kind is open
    t.stereoKeyframeBegin(B, s.rp, do, s.skp)
    f0 = items[0]["frame"]
    for call in (lambda: t.stereoKeyframeBegin(B, s.rp, do, s.skp), lambda: t.trackMonoResidentBegin([it["left2"] for it in items], *a1),
                 lambda: t.createKeyframeBegin(B, None, None, None, None, np.zeros(B, np.uint8), s.nlmid.copy(), np.arange(B, dtype=np.int32),
                                               np.full(B, 11.0), _ckf_params(cfg, 0), s.state),
                 lambda: t.setFrame(0, f0["px"], f0["lmid"], f0["is3d"], f0["wpt"]), lambda: t.getFrame(0), lambda: t.updateFrame(1, [[]]),
                 lambda: t.setPose(0, items[0]["Twc"]), lambda: t.setKeyframeInfo(0, 1, 1.0, 1), lambda: t.getKeyframeInfo(0)):
        with pytest.raises(ov2slam_amd.Ov2Error) as err:
            call()
        assert err.value.code == L.OV2_EINVAL, str(err.value)
    assert lib.ov2_btracker_stereo_keyframe_end(t.h_trk, R5, None, None, None, None, None) == L.OV2_EINVAL          # still open afterwards
    recs, out = t.stereoKeyframeEnd()
    assert all(r["action"] == DONE for r in recs) and t.lastSlotBytes() == 0
    # ... and it did what the one call does on a fresh tracker (the log of the main scenario, first stereo call with everybody asked)
    after = s.views()
    assert after != before and after["device"] == after["mirror"] and after["info_device"] == after["info_mirror"]
    assert [i["kf_nb3dkps"] for i in after["info_device"]] == [r["nb3dkps"] for r in recs]
    # an open step refuses the call
    t.trackMonoResidentBegin([it["left2"] for it in items], *a1)
    refused(lambda: t.stereoKeyframe(B, s.rp, do, s.skp), "a step is open")
    t.trackMonoResidentEnd()
    # the step moved the frames on: nobody's frame is its keyframe any more
    recs, _ = t.stereoKeyframe(B, s.rp, do, s.skp)
    assert [r["action"] for r in recs] == [NOT_KEYFRAME] * B
    # update_frame: a SET keeps the keyframe, a REMOVE ends it
    s.ckf([1] * B, 0, 3, "ckf_again")
    fr = t.getFrame(0, False)
    if fr["n"] >= 2:
        t.updateFrame(1, [[(int(fr["lmid"][0]), L.OV2_RES_SET_POINT, (1.0, 2.0, 3.0))]])
        assert t.stereoKeyframe(1, s.rp, [1], s.skp)[0][0]["action"] == DONE
        t.updateFrame(1, [[(int(fr["lmid"][1]), L.OV2_RES_REMOVE, None)]])
        assert t.stereoKeyframe(1, s.rp, [1], s.skp)[0][0]["action"] == NOT_KEYFRAME
    t.close()
    s.rp.close()


def _changed(ctx, S, **kw):
    """the scenario's params struct with one field changed (tri_<field>: inside the embedded ov2_tri_params; a pose field: its first
    entry)"""
    p = R.skf_params(ctx, S)
    for k, v in kw.items():
        tgt, f = (p.tri, k[4:]) if k.startswith("tri_") else (p, k)
        if f in ("Tcic0", "Tlr"):
            getattr(tgt, f)[0] = v
        else:
            setattr(tgt, f, v)
    return p


def _regrow_play(ctx, name, one_cell_first):
    """the scenario up to its keyframes, [a call that asks nobody on a grid of one cell: the block at that size], the scenario's call
    (11 x 7 cells) and a call on a coarser grid (6 x 4 cells) -> one entry per stereo call: records, outputs, the four views"""
    s = _Side(ctx, name, "B", "one")
    S, cfg, B, t = s.S, s.cfg, s.B, s.t
    items = S["items"]
    for b in range(B):
        t.setPose(b, items[b]["Twc"])
        s.set_frame(b, items[b]["frame"])
    s.step([it["left"] for it in items], 0, "first_frame")
    nbw, nbh = _grid(cfg)
    s.ckf([1] * B, nbw * nbh, 0, "ckf_main")
    log = []

    def call(do, params):
        recs, out = t.stereoKeyframe(B, s.rp, do, params, out=R.empty_out(B, N_MAX, POISON))
        log.append(dict(recs=recs, out=out, views=s.views(), slot_bytes=t.lastSlotBytes()))
        return log[-1]

    if one_cell_first:
        before = s.views()
        e = call([0] * B, _changed(ctx, S, ncellsize=4 * cfg["w"]))
        assert [r["action"] for r in e["recs"]] == [NOT_REQUESTED] * B and e["views"] == before
        assert all((a.view(np.uint8) == POISON).all() for a in e["out"].values())
        log.clear()
    call([1] * B, s.skp)
    call([1] * B, _changed(ctx, S, ncellsize=2 * CELL))
    t.close()
    s.rp.close()
    return log


def test_a_regrown_block_changes_nothing(gpu_ctx):
    """The call's device block is regrown, with a new layout, when a call's grid has more cells than any before.  Tracker A's first
    call asks nobody on a grid of one cell (the block at that size; nothing changes), its second is the scenario's call (77 cells: the
    block is regrown), its third has a coarser grid (24 cells: the block stays).  Tracker B makes the two real calls only.  Every
    record, every output array and the frame and the keyframe info, from the device and from the mirror, are byte-equal."""
    name = "unrect-radtan"
    cfg = R.CONFIGS[name]
    assert int(np.ceil(cfg["w"] / (4 * cfg["w"]))) * int(np.ceil(cfg["h"] / (4 * cfg["w"]))) == 1
    assert 1 < int(np.ceil(cfg["w"] / (2 * CELL))) * int(np.ceil(cfg["h"] / (2 * CELL))) < _grid(cfg)[0] * _grid(cfg)[1]
    A, B = _regrow_play(gpu_ctx, name, True), _regrow_play(gpu_ctx, name, False)
    assert len(A) == len(B) == 2
    for i, (a, b) in enumerate(zip(A, B)):
        assert a["recs"] == b["recs"], (i, a["recs"], b["recs"])
        assert all(r["action"] == DONE for r in a["recs"]) and a["slot_bytes"] == b["slot_bytes"] == 0
        for k in a["out"]:
            assert a["out"][k].tobytes() == b["out"][k].tobytes(), (i, k)
        assert a["views"] == b["views"], i
        assert a["views"]["device"] == a["views"]["mirror"] and a["views"]["info_device"] == a["views"]["info_mirror"], i
    assert sum(r["n_stereo_good"] for r in A[0]["recs"]) >= 5 and sum(r["n_prior_nb"] for r in A[0]["recs"]) >= 10
