"""ov2_btracker_temporal_keyframe (scope row f23; csrc/temporalkf.hip, csrc/trackb_keyframe.hip): Mapper::triangulateTemporal on the resident
keyframe in one lock-step call, against the route of separate calls it replaces (tests/temporalkf_ref.py: route, with the host anchor
walk).  Tracker A plays the script through the route, tracker B through the new call, once as one call and once as two halves.  EVERY
comparison is on raw bytes: both sides run the same device arithmetic on the same inputs, so equality is the requirement, not a tolerance.
Compared after every call: every field of every record, the four per-slot outputs (scattered into poisoned arrays: what a call does not
write stays poison on both sides), getFrame, getKeyframeInfo and getAnchors from the device and from the mirror, lastSlotBytes() == 0 on
B; and after every keyframe a trackMonoResident step on both trackers, whose filter reads the resident keyframe the call compacted and
whose decision reads the new kf_nb3dkps.

Shapes: 376 x 240 mono pinhole and 161 x 121 stereo fisheye (behind a stereoKeyframe), no CLAHE, batch 4, 160 slots, 8 rows.  The cycle
runs three keyframes of the script: setFrame -> createKeyframe(px=None) -> temporalKeyframe -> trackMonoResident.  What the script makes
the triangulation do is asserted without a GPU in tests/test_temporalkf_reference.py."""
import numpy as np
import pytest

import ov2slam_amd
from ov2slam_amd import _lib as L
from ov2slam_amd import mapper
from tests import resident_ref as RR
from tests import stereokf_ref as SR
from tests import temporalkf_ref as R
from tests.test_gpu_stereokf import _ckf_params, _step_args
from tests.test_gpu_trackmono import _same_mono_step

pytestmark = pytest.mark.gpu

POISON = 0x5A
N_MAX = R.N_MAX
NOT_REQUESTED, NOT_KEYFRAME, DONE, SRC_OVERFLOW = R.NOT_REQUESTED, R.NOT_KEYFRAME, R.DONE, R.SRC_OVERFLOW
ZERO = dict.fromkeys(R.REC_KEYS, 0)
_RUNS = {}


def _anchor_bytes(a):
    return {k: (v if isinstance(v, int) else np.ascontiguousarray(v).tobytes()) for k, v in a.items()}


class _Side:
    """one tracker and the bookkeeping of the script: which items' frames are their keyframes, the keyframes, the points made so far,
    and on side A the anchor tables of the host walk"""

    def __init__(self, ctx, name, which, how, n_src_max=R.N_SRC_MAX):
        self.ctx, self.S, self.which, self.how, self.ns = ctx, R.script(name), which, how, n_src_max
        cfg = self.cfg = self.S["cfg"]
        self.B = cfg["batch"]
        self.t = ov2slam_amd.LockstepTracker(ctx, self.B, cfg["w"], cfg["h"], use_clahe=False, nbmaxkps=N_MAX)
        self.t.setCalibration(SR.calibrations(ctx, self.S)[0])
        self.t.reserveAnchors(n_src_max)
        self.tkp = mapper.temporal_keyframe_params(self.S["tri"], n_src_max=n_src_max)
        self.imgs = [SR.pair(cfg, b) for b in range(self.B)]
        self.imgs2 = [SR.pair(cfg, b, (2, 1))[0] for b in range(self.B)]
        self.rp = self.skp = None
        if cfg["stereo"]:
            self.skp = SR.skf_params(ctx, self.S)
            self.rp = ov2slam_amd.Pyramid(ctx, cfg["w"], cfg["h"], SR.WIN, 3, batch=self.B).build(np.stack([p[1] for p in self.imgs]))
        self.iskf = [False] * self.B
        self.kf = [None] * self.B
        self.tables = [R.AnchorTable() for _ in range(self.B)]
        self.known = [dict() for _ in range(self.B)]
        self.state = np.full(self.B, 1e-3, np.float64)
        self.log = []

    def close(self):
        self.t.close()
        if self.rp is not None:
            self.rp.close()

    def views(self):
        t, B = self.t, self.B
        return dict(device=[RR.frame_bytes(t.getFrame(b, True)) for b in range(B)], mirror=[RR.frame_bytes(t.getFrame(b, False)) for b in range(B)],
                    info_device=[t.getKeyframeInfo(b, True) for b in range(B)], info_mirror=[t.getKeyframeInfo(b, False) for b in range(B)],
                    anc_device=[_anchor_bytes(t.getAnchors(b, True)) for b in range(B)], anc_mirror=[_anchor_bytes(t.getAnchors(b, False)) for b in range(B)])

    def note(self, kind, **kw):
        self.log.append(dict(kind=kind, views=self.views(), **kw))
        return self.log[-1]

    def set_frame(self, b, f):
        self.t.setFrame(b, f["px"], f["lmid"], f["is3d"], f["wpt"])
        self.iskf[b] = False

    def ckf(self, k, tag):
        B = self.B
        ids = np.array([R.kfid_of(k, b) for b in range(B)], np.int32)
        times = np.full(B, 10.01 + k)
        recs, o = self.t.createKeyframe(B, None, None, None, None, np.ones(B, np.uint8), np.full(B, 100000, np.int32), ids, times,
                                        _ckf_params(self.cfg, 0), self.state)
        for b, r in enumerate(recs):
            assert r["action"] == L.OV2_CKF_CREATED and r["n_new"] == 0, r
            n = r["n_kf"]
            order = np.argsort(o["lmid"][b, :n], kind="stable")
            self.iskf[b] = True
            self.kf[b] = dict(id=int(ids[b]), time=float(times[b]), Twc=self.t.getPose(b), lmid=o["lmid"][b, :n][order].copy(),
                              unpx=o["unpx"][b, :n][order].copy(), bv=o["bv"][b, :n][order].copy())
        return self.note(tag, ckf=recs)

    def skf(self, tag):
        """the stereo block in front of the temporal one: the same call on both sides"""
        recs, out = self.t.stereoKeyframe(self.B, self.rp, [1] * self.B, self.skp)
        for b, r in enumerate(recs):
            lm = self.t.getFrame(b, False)["lmid"]
            for i in np.nonzero(out["tri_status"][b, :r["n"]] & L.OV2_TRI_STEREO_OK)[0]:
                self.known[b][int(lm[i])] = out["wpt"][b, i].copy()
        return self.note(tag, skf=recs)

    def tkf(self, do, tag):
        na = len(do)
        actions = [NOT_REQUESTED if not do[b] else (DONE if self.iskf[b] else NOT_KEYFRAME) for b in range(na)]
        out = R.empty_out(self.B, N_MAX, POISON)
        if self.which == "A":
            recs, out = R.route(self.ctx, self.t, na, actions, self.S["tri"], self.ns, self.kf, self.tables, out)
            slot_bytes = None
        else:
            if self.how == "one":
                recs, out = self.t.temporalKeyframe(na, do, self.tkp, out=out)
            else:
                self.t.temporalKeyframeBegin(na, do, self.tkp)
                recs, out = self.t.temporalKeyframeEnd(out=out)
            slot_bytes = self.t.lastSlotBytes()
        for b, r in enumerate(recs):
            assert r["action"] == actions[b] or (actions[b] == DONE and r["action"] == SRC_OVERFLOW), (tag, b, r, actions)
            if r["action"] != DONE:
                continue
            lm = self.t.getFrame(b, False)["lmid"]
            for i in np.nonzero(out["tri_status"][b, :r["n"]] & R.OK)[0]:
                self.known[b][int(lm[i])] = out["wpt"][b, i].copy()
        return self.note(tag, do=list(do), recs=recs, out=out, slot_bytes=slot_bytes)

    def move_pose(self, triples, tag):
        """local BA moved keyframes: side A changes its tables and installs them, side B sends the triples"""
        if self.which == "A":
            ignored = 0
            for b, kfid, T in triples:
                ignored += self.tables[b].set_poses([(kfid, T)])
            for b in sorted({x[0] for x in triples}):
                tb = self.tables[b]
                self.t.setAnchors(b, tb.lmid, tb.kfid, tb.unpx, tb.bv, tb.row_kfid, tb.row_Twc)
        else:
            ignored = self.t.setAnchorPoses(triples)
        return self.note(tag, ignored=ignored)

    def step(self, imgs, f, tag):
        t, B = self.t, self.B
        nb = [t.getFrame(b, False)["n"] for b in range(B)]
        out, st, rule, epis, poses, monos, frames = t.trackMonoResident(imgs, *_step_args(self.S, f))
        for b in range(B):
            self.iskf[b] = False
        nk = [0] * B if f == 0 else nb                                    # the tracker's first frame tracks nothing
        rec = dict(out=out, st=st, rule=rule, epis=epis, poses=poses, monos=monos, frames=frames,
                   res_T=np.array([t.getPose(b) for b in range(B)]), res_s=[t.getMotion(b) for b in range(B)],
                   kp=[t.lastKeypoints(b, nk[b]) for b in range(B)], pr=[t.lastPriors(b, nk[b]) for b in range(B)],
                   inputs=[t.lastPoseInputs(b) for b in range(B)], einputs=[t.lastEpiInputs(b) for b in range(B)])
        return self.note(tag, nb=nb, **rec)


def _play(ctx, name, which, how="one", n_src_max=R.N_SRC_MAX):
    """three keyframes of the script on a fresh tracker: side 'A' (the route) or 'B' (the new call; how: 'one' call or two 'halves')
    -> the log, one entry per call.  Computed once per key and shared; nobody changes a result."""
    key = (name, which, how, n_src_max)
    if key in _RUNS:
        return _RUNS[key]
    s = _Side(ctx, name, which, how, n_src_max)
    S, B, t = s.S, s.B, s.t
    items = S["items"]
    for b in range(B):
        t.setPose(b, items[b]["poses"][0])
        s.set_frame(b, R.frame_for(items[b], 0, s.known[b]))
    s.step([p[0] for p in s.imgs], 0, "first_frame")                    # the tracker's first frame: the frames stay
    for k in range(3):
        if k == 2:                                                       # local BA moved keyframe 0 of items 0 and 1; keyframe 999 is nobody's
            moved = [items[b]["poses"][0] + np.array([0.004, -0.003, 0.002, 0, 0, 0, 0]) for b in range(2)]
            s.move_pose([(0, R.kfid_of(0, 0), moved[0]), (1, R.kfid_of(0, 1), moved[1]), (2, 999, moved[0])], "ba")
        for b in range(B):
            t.setPose(b, items[b]["poses"][k])
            s.set_frame(b, R.frame_for(items[b], k, s.known[b]))
        s.ckf(k, "ckf%d" % k)
        if s.cfg["stereo"]:
            s.skf("skf%d" % k)
        if k == 0:
            s.tkf([0] * B, "nobody")                                     # do = 0: everything stays
            s.tkf([1] * B, "kf0")
        elif k == 1:
            s.tkf([1, 1, 1, 0], "kf1")                                   # item 3 is not asked
            s.tkf([1] * B, "kf1_again")                                  # a second call on the same keyframe; item 3's first
            s.tkf([0, 1, 1], "three_of_four")                            # n_active 3: item 3 is not looked at
        else:
            s.tkf([1] * B, "kf2")
            s.set_frame(1, t.getFrame(1, False))                         # item 1's frame is installed again: no longer its keyframe
            s.note("set_frame_again")
            s.tkf([1] * B, "after_set_frame")
        s.step(s.imgs2 if k % 2 == 0 else [p[0] for p in s.imgs], k + 1, "step%d" % k)
    s.close()
    _RUNS[key] = s.log
    return s.log


def _same_log(A, B, where):
    assert [e["kind"] for e in A] == [e["kind"] for e in B]
    for i, (a, b) in enumerate(zip(A, B)):
        at = (where, i, a["kind"])
        if "monos" in a:
            _same_mono_step(a, b, at)
            assert a["frames"] == b["frames"] and a["nb"] == b["nb"], (at, a["frames"], b["frames"])
        elif "recs" in a:
            assert a["recs"] == b["recs"], (at, a["recs"], b["recs"])
            for k in a["out"]:
                assert a["out"][k].tobytes() == b["out"][k].tobytes(), (at, k)
            assert b["slot_bytes"] == 0, (at, b["slot_bytes"])
        elif "ckf" in a:
            assert a["ckf"] == b["ckf"], (at, a["ckf"], b["ckf"])
        elif "skf" in a:
            assert a["skf"] == b["skf"], (at, a["skf"], b["skf"])
        elif "ignored" in a:
            assert a["ignored"] == b["ignored"] == 1, (at, a["ignored"], b["ignored"])
        # A's device block, A's mirror, B's device block and B's mirror hold the same bytes: frames, keyframe info, anchors
        for dev, mir in (("device", "mirror"), ("info_device", "info_mirror"), ("anc_device", "anc_mirror")):
            for item in range(len(a["views"][dev])):
                x = a["views"][dev][item]
                for view in (dev, mir):
                    y = b["views"][view][item]
                    for k in x:
                        assert x[k] == y[k], (at, "item %d" % item, view, k)
                assert x == a["views"][mir][item], (at, "A's own mirror", dev, item)


def _show(name, A):
    for e in A:
        if "monos" in e:
            print(name, e["kind"], "frames", [(f["n_before"], f["n_after"]) for f in e["frames"]],
                  "kf", [(m["kf"]["n"], m["kf"]["nb3dkps"], m["kf"]["decision"], m["kf"]["reason"]) for m in e["monos"]])
        elif "recs" in e:
            print(name, e["kind"], e["do"], [tuple(r[k] for k in R.REC_KEYS) for r in e["recs"]])


@pytest.mark.parametrize("how", ["one", "halves"])
@pytest.mark.parametrize("name", sorted(R.CONFIGS))
def test_the_call_equals_the_route(gpu_ctx, name, how):
    A, B = _play(gpu_ctx, name, "A"), _play(gpu_ctx, name, "B", how)
    _show(name, A)
    _same_log(A, B, (name, how))


@pytest.mark.parametrize("name", sorted(R.CONFIGS))
def test_the_route_takes_every_branch(gpu_ctx, name):
    """on A's side alone: the three keyframes reach what they were built for"""
    A = _play(gpu_ctx, name, "A")
    _show(name, A)
    by = {e["kind"]: e for e in A}
    same_item = lambda x, y, b: all(x["views"][v][b] == y["views"][v][b] for v in x["views"])
    prev = lambda kind: A[[e["kind"] for e in A].index(kind) - 1]
    # do = 0: nothing is read or written
    nobody = by["nobody"]
    assert nobody["recs"] == [dict(ZERO, action=NOT_REQUESTED)] * 4 and nobody["views"] == prev("nobody")["views"]
    assert all((a.view(np.uint8) == POISON).all() for a in nobody["out"].values())
    # keyframe 0: everybody anchors there, nobody is a candidate
    r0 = by["kf0"]["recs"]
    assert all(r["action"] == DONE and r["n_candidates"] == 0 and r["n_rows"] == 1 for r in r0) and [r0[3]["n"]] == [0]
    # keyframe 1: candidates, new points, keypoints taken out of the keyframe; item 3 is not asked, and keeps everything
    mono = name == "mono-pinhole"
    k1 = by["kf1"]
    r1 = k1["recs"]
    tot = {k: sum(r[k] for r in r1) for k in R.REC_KEYS}
    assert tot["n_candidates"] > tot["n_temporal_good"] >= 5 and tot["n_remove_obs"] >= 1
    assert r1[3] == dict(ZERO, action=NOT_REQUESTED) and same_item(k1, prev("kf1"), 3)
    assert all((a[3].view(np.uint8) == POISON).all() for a in k1["out"].values())
    for b in range(3):
        r, n = r1[b], r1[b]["n"]
        st = k1["out"]["tri_status"][b, :n]
        assert r["n_rows"] == 2
        if mono:                                                         # (in stereo the block in front has made most slots 3-D)
            assert r["n_candidates"] >= 10 and r["n_remove_obs"] >= 1 and r["n_temporal_good"] >= 5
        before = np.frombuffer(prev("kf1")["views"]["device"][b]["is3d"], np.uint8)
        after = np.frombuffer(k1["views"]["device"][b]["is3d"], np.uint8)
        good = (st & R.OK) != 0
        assert np.array_equal(after, before | good) and r["nb3dkps"] == int(after.sum()) == k1["views"]["info_device"][b]["kf_nb3dkps"]
        assert not (good & (before != 0)).any() and ((k1["out"]["src_kfid"][b, :n] >= 0) >= ((st & R.TRIED) != 0)).all()
        assert np.isfinite(k1["out"]["wpt"][b, :n]).all() and not k1["out"]["wpt"][b, :n][~good].any()
        assert all((a[b, n:].view(np.uint8) == POISON).all() for a in k1["out"].values())
        assert k1["views"]["anc_device"][b]["n"] == n                    # the table keeps the keypoints the keyframe lost
    # the second call on keyframe 1: the anchors stay, the removed keypoints are no candidates any more, nothing is made or removed
    again = by["kf1_again"]
    for b in range(3):
        r = again["recs"][b]
        assert r["action"] == DONE and r["n_temporal_good"] == 0 and r["n_remove_obs"] == 0 and r["n_candidates"] <= r1[b]["n_candidates"] - r1[b]["n_remove_obs"] - r1[b]["n_temporal_good"]
        assert again["views"]["anc_device"][b] == k1["views"]["anc_device"][b] and again["views"]["device"][b] == k1["views"]["device"][b]
    assert again["recs"][3]["action"] == DONE and again["recs"][3]["n"] == 1 and again["recs"][3]["n_candidates"] == 0
    three = by["three_of_four"]
    assert len(three["recs"]) == 3 and [r["action"] for r in three["recs"]] == [NOT_REQUESTED, DONE, DONE] and same_item(three, again, 3)
    # local BA: the two rows moved on both copies, the third triple anchors nothing
    ba = by["ba"]
    for b in range(2):
        got = np.frombuffer(ba["views"]["anc_device"][b]["row_Twc"], np.float64).reshape(-1, 7)
        ids = np.frombuffer(ba["views"]["anc_device"][b]["row_kfid"], np.int32)
        was = np.frombuffer(prev("ba")["views"]["anc_device"][b]["row_Twc"], np.float64).reshape(-1, 7)
        at = int(np.nonzero(ids == R.kfid_of(0, b))[0][0])
        assert np.array_equal(got[at, :3], was[at, :3] + np.array([0.004, -0.003, 0.002])) and np.array_equal(np.delete(got, at, 0), np.delete(was, at, 0))
        assert ba["views"]["anc_device"][b]["row_Tcw"] != prev("ba")["views"]["anc_device"][b]["row_Tcw"]
    assert same_item(ba, prev("ba"), 2) and same_item(ba, prev("ba"), 3)
    # keyframe 2: points anchored at the moved keyframe 0 are made with its new pose (the route hands that pose to the triangulation)
    k2 = by["kf2"]
    for b in range(2 if mono else 0):
        n = k2["recs"][b]["n"]
        from0 = (k2["out"]["src_kfid"][b, :n] == R.kfid_of(0, b)) & ((k2["out"]["tri_status"][b, :n] & R.TRIED) != 0)
        assert from0.any(), (b, "no candidate anchored at keyframe 0")
    assert k2["recs"][3]["n"] >= 2 and k2["recs"][3]["nb3dkps"] == k2["recs"][3]["n"] and k2["recs"][3]["n_candidates"] == 0      # every slot 3-D
    assert max(r["n_rows"] for r in k2["recs"]) == 3
    # item 1 stands still between keyframes 1 and 2: in stereo mode its candidates anchored at keyframe 1 are skipped, in mono never
    assert (k2["recs"][1]["n_no_motion"] >= 1) == (not mono) and all(r["n_no_motion"] == 0 for e in A if "recs" in e for b, r in enumerate(e["recs"]) if mono or b != 1)
    # after setFrame: NOT_KEYFRAME, nothing written; the others run a second time
    after = by["after_set_frame"]
    assert after["recs"][1] == dict(ZERO, action=NOT_KEYFRAME) and same_item(after, by["set_frame_again"], 1)
    assert all((a[1].view(np.uint8) == POISON).all() for a in after["out"].values())
    assert [after["recs"][b]["action"] for b in (0, 2, 3)] == [DONE] * 3
    # the step behind every keyframe tracked something
    assert all(sum(f["n_before"] for f in by["step%d" % k]["frames"]) > 0 for k in range(3))
    if name == "stereo-fisheye":
        assert all(r["action"] == L.OV2_SKF_DONE for k in range(3) for r in by["skf%d" % k]["skf"])


def test_src_overflow_leaves_everything_where_it_was(gpu_ctx):
    """two rows: the third keyframe in a row with births overflows for the items whose points of keyframes 0 and 1 live on.  Frame,
    keyframe info and anchors are byte-equal before and after, on the device and in the mirror, on the route's side and the call's"""
    name = "mono-pinhole"
    A, B = _play(gpu_ctx, name, "A", "one", 2), _play(gpu_ctx, name, "B", "one", 2)
    _same_log(A, B, (name, "two rows"))
    kinds = [e["kind"] for e in B]
    k2, before = B[kinds.index("kf2")], B[kinds.index("kf2") - 1]
    acts = [r["action"] for r in k2["recs"]]
    assert acts[:3] == [SRC_OVERFLOW] * 3 and acts[3] == DONE, acts
    for b in range(3):
        assert k2["recs"][b] == dict(ZERO, action=SRC_OVERFLOW)
        assert all(k2["views"][v][b] == before["views"][v][b] for v in k2["views"])
        assert all((a[b].view(np.uint8) == POISON).all() for a in k2["out"].values())
    assert all(r["n_rows"] <= 2 for e in B if "recs" in e for r in e["recs"])
    # the step behind it saw the keyframes as they were: equal on both sides (compared above), and it ran
    assert sum(f["n_before"] for f in B[kinds.index("step2")]["frames"]) > 0


def test_refusals_leave_the_tracker_where_it_was(gpu_ctx):
    """every OV2_EINVAL of the calls returns before the tracker changes (frame, info and anchors byte-equal before and after); while a
    call is open a second _begin, a step's _begin and the calls around the resident state are refused"""
    name = "mono-pinhole"
    s = _Side(gpu_ctx, name, "B", "one")
    S, cfg, B, t = s.S, s.cfg, s.B, s.t
    items = S["items"]

    def refused(call, words, code=L.OV2_EINVAL):
        with pytest.raises(ov2slam_amd.Ov2Error) as err:
            call()
        assert err.value.code == code and words in str(err.value), (words, str(err.value))

    do = [1] * B
    # a tracker without a resident frame; without an anchor block; the block comes with the first call, another n_src_max is refused
    t2 = ov2slam_amd.LockstepTracker(gpu_ctx, B, cfg["w"], cfg["h"], use_clahe=False, nbmaxkps=N_MAX)
    refused(lambda: t2.temporalKeyframe(B, do, s.tkp), "no resident frame")
    refused(lambda: t2.getAnchors(0), "no anchor block")
    refused(lambda: t2.setAnchorPoses([(0, 1, items[0]["poses"][0])]), "no anchor block")
    f = R.frame_for(items[0], 0, {})
    t2.setFrame(0, f["px"], f["lmid"], f["is3d"], f["wpt"])
    refused(lambda: t2.temporalKeyframe(B, do, mapper.temporal_keyframe_params(S["tri"], n_src_max=0)), "n_src_max outside")
    refused(lambda: t2.temporalKeyframe(B, do, mapper.temporal_keyframe_params(S["tri"], n_src_max=L.OV2_TKF_MAX_ROWS + 1)), "n_src_max outside")
    recs, _ = t2.temporalKeyframe(B, do, s.tkp)                            # nobody's frame is a keyframe; the block exists now
    assert [r["action"] for r in recs] == [NOT_KEYFRAME] * B and t2.getAnchors(0, True)["n"] == 0
    refused(lambda: t2.temporalKeyframe(B, do, mapper.temporal_keyframe_params(S["tri"], n_src_max=4)), "n_src_max differs")
    refused(lambda: t2.reserveAnchors(4), "n_src_max differs")
    t2.close()
    for b in range(B):
        t.setPose(b, items[b]["poses"][0])
        s.set_frame(b, R.frame_for(items[b], 0, {}))
    s.step([p[0] for p in s.imgs], 0, "first_frame")
    s.ckf(0, "ckf0")
    s.tkf(do, "kf0")
    for b in range(B):
        t.setPose(b, items[b]["poses"][1])
        s.set_frame(b, R.frame_for(items[b], 1, {}))
    s.ckf(1, "ckf1")
    before = s.views()
    bad = lambda **kw: _changed(S, **kw)
    refused(lambda: t.temporalKeyframe(0, do, s.tkp), "n_active out of range")
    refused(lambda: t.temporalKeyframe(B + 1, do + [1], s.tkp), "n_active out of range")
    refused(lambda: t.temporalKeyframe(B, do, bad(n_src_max=4)), "n_src_max differs")
    refused(lambda: t.temporalKeyframe(B, do, bad(K=np.nan)), "tri.K not finite")
    refused(lambda: t.temporalKeyframe(B, do, bad(Tlr=np.nan)), "pose not finite")
    refused(lambda: t.temporalKeyframe(B, do, bad(Tcic0=np.inf)), "pose not finite")
    lib = t.lib
    R4 = (L.TemporalKeyframeResult * B)()
    dob = np.ones(B, np.uint8)
    assert lib.ov2_btracker_temporal_keyframe_begin(t.h_trk, B, None, dob.ctypes.data) == L.OV2_EINVAL
    assert lib.ov2_btracker_temporal_keyframe_begin(t.h_trk, B, s.tkp, None) == L.OV2_EINVAL
    assert lib.ov2_btracker_temporal_keyframe_end(t.h_trk, R4, None, None, None, None) == L.OV2_EINVAL
    assert b"without ov2_btracker_temporal_keyframe_begin" in lib.ov2_last_error()
    assert lib.ov2_btracker_temporal_keyframe(t.h_trk, B, s.tkp, dob.ctypes.data, None, None, None, None, None) == L.OV2_EINVAL
    # set_anchors: the table of item 0 as it is, with one thing wrong at a time
    a = t.getAnchors(0, False)
    good = (a["lmid"], a["kfid"], a["unpx"], a["bv"], a["row_kfid"], a["row_Twc"])
    assert a["n"] >= 3 and a["n_rows"] == 1
    sa = lambda i, v, item=0: (lambda: t.setAnchors(item, *[v if j == i else x for j, x in enumerate(good)]))
    refused(sa(0, a["lmid"][::-1].copy()), "lmid unsorted")
    refused(sa(0, np.concatenate([a["lmid"][:1], a["lmid"][:-1]])), "lmid unsorted")
    refused(sa(1, a["kfid"] + 1), "not among the rows")
    refused(sa(3, np.where(np.arange(a["n"])[:, None] == 1, np.nan, a["bv"])), "not finite")
    refused(sa(5, a["row_Twc"] * np.nan), "pose not finite")
    refused(lambda: t.setAnchors(0, a["lmid"], a["kfid"], a["unpx"], a["bv"], [a["row_kfid"][0], a["row_kfid"][0]], np.tile(a["row_Twc"], (2, 1))), "row_kfid unsorted")
    refused(lambda: t.setAnchors(0, *[np.concatenate([x] * (N_MAX // a["n"] + 1)) for x in good[:4]], a["row_kfid"], a["row_Twc"]), "n outside")
    refused(lambda: t.setAnchors(0, *good[:4], np.arange(R.N_SRC_MAX + 1), np.tile(a["row_Twc"], (R.N_SRC_MAX + 1, 1))), "n_rows outside")
    refused(lambda: t.setAnchors(B, *good), "batch item out of range")
    refused(lambda: t.getAnchors(-1), "batch item out of range")
    # set_anchor_poses
    T0 = items[0]["poses"][0]
    refused(lambda: t.setAnchorPoses([(B, 1, T0)]), "batch item out of range")
    refused(lambda: t.setAnchorPoses([(0, 1, T0), (0, 1, T0)]), "twice")
    refused(lambda: t.setAnchorPoses([(0, 1, T0 * np.nan)]), "pose not finite")
    refused(lambda: t.setAnchorPoses([(b % B, k, T0) for b in range(B) for k in range(R.N_SRC_MAX + 1)]), "n outside")
    assert t.setAnchorPoses([]) == 0 and t.setAnchorPoses([(0, 12345, T0)]) == 1
    assert s.views() == before and t.lastSlotBytes() == 0
    # a table that knows a keyframe newer than the resident one
    t.setAnchors(0, a["lmid"], a["kfid"] + 1000, a["unpx"], a["bv"], a["row_kfid"] + 1000, a["row_Twc"])
    refused(lambda: t.temporalKeyframe(B, do, s.tkp), "newer than its resident keyframe")
    t.setAnchors(0, *good)
    assert s.views() == before
    # an open createKeyframe call, an open step
    a1 = _step_args(S, 1)
    ckf_begin = lambda: t.createKeyframeBegin(B, None, None, None, None, np.zeros(B, np.uint8), np.full(B, 100000, np.int32), np.arange(B, dtype=np.int32),
                                              np.full(B, 11.0), _ckf_params(cfg, 0), s.state)
    ckf_begin()
    refused(lambda: t.temporalKeyframe(B, do, s.tkp), "create_keyframe_begin has not been finished")
    t.createKeyframeEnd()
    assert s.views() == before
    # while a call of this kind is open
    t.temporalKeyframeBegin(B, do, s.tkp)
    f0 = R.frame_for(items[0], 0, {})
    for call in (lambda: t.temporalKeyframeBegin(B, do, s.tkp), lambda: t.trackMonoResidentBegin(s.imgs2, *a1), ckf_begin,
                 lambda: t.setFrame(0, f0["px"], f0["lmid"], f0["is3d"], f0["wpt"]), lambda: t.getFrame(0), lambda: t.updateFrame(1, [[]]),
                 lambda: t.setPose(0, T0), lambda: t.setKeyframeInfo(0, 1, 1.0, 1), lambda: t.getKeyframeInfo(0), lambda: t.setAnchors(0, *good),
                 lambda: t.getAnchors(0), lambda: t.setAnchorPoses([(0, 1, T0)]), lambda: t.reserveAnchors(R.N_SRC_MAX),
                 lambda: t.setKeyframe(0, a["lmid"], a["unpx"], a["bv"], T0)):
        with pytest.raises(ov2slam_amd.Ov2Error) as err:
            call()
        assert err.value.code == L.OV2_EINVAL, str(err.value)
    assert lib.ov2_btracker_temporal_keyframe_end(t.h_trk, R4, None, None, None, None) == L.OV2_EINVAL          # still open afterwards
    recs, out = t.temporalKeyframeEnd()
    assert all(r["action"] == DONE for r in recs) and t.lastSlotBytes() == 0
    after = s.views()
    assert after != before and all(after[d] == after[m] for d, m in (("device", "mirror"), ("info_device", "info_mirror"), ("anc_device", "anc_mirror")))
    assert [i["kf_nb3dkps"] for i in after["info_device"]] == [r["nb3dkps"] for r in recs]
    # an open step refuses the call; the step moves the frames on: nobody's frame is its keyframe any more
    t.trackMonoResidentBegin(s.imgs2, *a1)
    refused(lambda: t.temporalKeyframe(B, do, s.tkp), "a step is open")
    t.trackMonoResidentEnd()
    recs, _ = t.temporalKeyframe(B, do, s.tkp)
    assert [r["action"] for r in recs] == [NOT_KEYFRAME] * B
    s.close()


def _changed(S, **kw):
    """the script's params struct with one field changed (a pose or K: its first entry)"""
    p = mapper.temporal_keyframe_params(S["tri"], n_src_max=R.N_SRC_MAX)
    for k, v in kw.items():
        if k == "n_src_max":
            p.n_src_max = v
        else:
            getattr(p.tri, k)[0] = v
    return p
