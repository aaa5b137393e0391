"""Tracking from the keyframe in the lock-step step (ov2_btracker_set_track_from_keyframe; csrc/kltkf.hip, lkw_kf.hip, lk.hip):
VisualFrontEnd::kltTrackingFromKF of the reference.
  * the keyframe store: k_kfpyr_adopt copies the whole item stride of the flagged items and leaves the others alone (compared through
    a device-to-host copy of both pyramids' items); the px table is perm / px of create_keyframe's own outputs, on the device and in
    the host mirror;
  * the epi_pose, mono and resident mono step forms with the mode on, on every case of tests/kltfromkf_cases.py with and without
    CLAHE: out_xy bit-equal and status / p3p_req equal to tests/kltfromkf_ref.py on oracle pyramids, and byte-equal to the route of
    separate calls on the device (the host join and ov2_fb_klt twice on kf_item / cur_item); a slot whose id was taken out of the
    resident keyframe's list (what ov2_btracker_temporal_keyframe does on REMOVE_OBS) or that the table never held comes out with
    status 4 and its input px;
  * the resident cycle keyframe -> 3 frames -> keyframe -> 2 frames against the same cycle on host-kept frames (the sides of
    tests/test_gpu_resident.py on trackers of 5 items of which 4 take part), byte for byte; the second keyframe replaces the store;
  * mode off after on equals a tracker that never had it on; the refusals enqueue nothing and leave the state as it was.
Frame size and slots: those of tests/test_gpu_resident.py; batch 5, 4 active."""
import numpy as np
import pytest

import ov2slam_amd
from ov2slam_amd import _lib as L
from ov2slam_amd import pose
from tests import createkf_ref as CR
from tests import kltfromkf_cases as KC
from tests import kltfromkf_ref as R
from tests import resident_ref as RR
from tests import test_gpu_resident as TR
from tests.test_gpu_frameepi import _epi_params
from tests.test_gpu_framepose import _params

pytestmark = pytest.mark.gpu

W, H, N_MAX, BATCH, NA = KC.W, KC.H, KC.N_MAX, KC.BATCH, KC.N_ACTIVE
I7 = np.array([0, 0, 0, 0, 0, 0, 1.0])
_STEPS = {}


def _cal(ctx):
    return ov2slam_amd.CameraCalibration(ctx, "pinhole", *KC.K)


def _tracker(ctx, clahe=False, on=True):
    t = ov2slam_amd.LockstepTracker(ctx, BATCH, W, H, use_clahe=clahe, nbmaxkps=N_MAX)
    t.setCalibration(_cal(ctx))
    if on:
        t.setTrackFromKeyframe(True)
    return t


def _slots(items):
    a = dict(px=np.zeros((BATCH, N_MAX, 2), np.float32), lmid=np.zeros((BATCH, N_MAX), np.int32), is3d=np.zeros((BATCH, N_MAX), np.uint8),
             wpt=np.zeros((BATCH, N_MAX, 3), np.float64), n=np.zeros(len(items), np.int32))
    for b, it in enumerate(items):
        n = it["n"]
        a["px"][b, :n], a["lmid"][b, :n], a["is3d"][b, :n], a["wpt"][b, :n], a["n"][b] = it["px"], it["lmid"], it["is3d"], it["wpt"], n
    return a


def _step(t, form, imgs, a, use_prior=True, f=1):
    """one step of the form on the frames `a` -> (out, status, p3p_req)"""
    na = len(imgs)
    Kc = KC.K
    seeds = np.arange(1, 2 * BATCH, 2).astype(np.uint64)
    pp, ep = _params(pose.LMEDS, True, Kc), _epi_params(False, True, Kc=Kc)
    zero, nb = np.zeros(BATCH, np.uint8), np.full(BATCH, 3, np.int32)
    tm, fid = np.full(BATCH, 10.0 + 0.05 * f), np.full(BATCH, f, np.int32)
    I = np.tile(I7, (BATCH, 1))
    if form == "epi_pose":
        r = t.trackFrameEpiPose(imgs, a["px"], a["wpt"], a["is3d"], I, a["n"], pp, ep, I, zero, seeds, a["lmid"], nb, seeds,
                                klt_use_prior=use_prior)
    elif form == "mono":
        r = t.trackMono(imgs, a["px"], a["wpt"], a["is3d"], a["n"], pp, ep, zero, seeds, a["lmid"], nb, seeds, tm, fid, klt_use_prior=use_prior)
    else:
        r = t.trackMonoResident(imgs, pp, ep, zero, seeds, nb, seeds, tm, fid, klt_use_prior=use_prior)
    return r[0], r[1], r[2]


def _install(t, cal, items, form):
    """the keyframes of the case: the first frame (the keyframe images), the resident keyframe list (the table's ids that are still
    members), the px table, the adopted pyramids; the identity pose, so that a 3-D point projects where the case designed it"""
    empty = _slots([dict(n=0, px=np.zeros((0, 2)), lmid=np.zeros(0), is3d=np.zeros(0), wpt=np.zeros((0, 3)))] * len(items))
    for b in range(len(items)):
        if form != "epi_pose":
            t.setPose(b, I7)
        if form == "resident":
            t.setFrame(b, np.zeros((0, 2)), np.zeros(0), np.zeros(0), np.zeros((0, 3)))
    _step(t, form, [it["kf_img"] for it in items], empty, f=0)
    for b, it in enumerate(items):
        m = it["members"]
        unpx, bv = cal.computeKeypoints(it["tab_px"][m]) if m.any() else (np.zeros((0, 2), np.float32), np.zeros((0, 3)))
        t.setKeyframe(b, it["tab_lmid"][m], unpx, bv, I7)
        t.setKeyframePx(b, it["tab_lmid"], it["tab_px"])
        if form != "epi_pose":
            t.setKeyframeInfo(b, 7, 10.0, 5)
            t.setPose(b, I7)
        if form == "resident":
            t.setFrame(b, it["px"], it["lmid"], it["is3d"], it["wpt"])
    t.adoptKeyframePyramid(len(items), np.ones(len(items), np.uint8))


def _run(ctx, name, form, clahe, impl="wave"):
    """the case's step on a fresh tracker -> dict, computed once per key and changed by nobody"""
    key = (name, form, clahe, impl)
    if key in _STEPS:
        return _STEPS[key]
    c = KC.case(name)
    items = c["items"]
    with ctx.options(track_impl=L.OV2_TRACK_IMPL_ROW if impl == "row" else L.OV2_TRACK_IMPL_WAVE):
        t, cal = _tracker(ctx, clahe), _cal(ctx)
        _install(t, cal, items, form)
        idle = dict(store=t.kf_item(BATCH - 1).download_item(), table=t.getKeyframePx(BATCH - 1, True))
        out, st, p3p = _step(t, form, [it["cur_img"] for it in items], _slots(items), c["use_prior"])
        pri = [t.lastPriors(b, it["n"]) for b, it in enumerate(items)]
        # the route of separate calls on the device: the host join, then ov2_fb_klt between the two item views, twice
        ft = ov2slam_amd.FeatureTracker(ctx, 30, 0.01)
        fb = lambda kp, cp, win, lvl, ferr, fbd, kps, pr, mi, eps: ft.fbKltTracking(kp, cp, win, lvl, ferr, fbd, kps, pr)
        route = []
        for b, it in enumerate(items):
            m = it["members"]
            route.append(R.klt_tracking_from_kf(t.kf_item(b), t.cur_item(b), it["px"], it["lmid"], it["tab_lmid"][m], it["tab_px"][m], pri[b][0],
                                                pri[b][1] & 1, klt_use_prior=c["use_prior"], fb=fb))
        idle_after = dict(store=t.kf_item(BATCH - 1).download_item(), table=t.getKeyframePx(BATCH - 1, True))
        t.close()
    _STEPS[key] = dict(case=c, out=out, st=st, p3p=p3p, pri=pri, route=route, idle=idle, idle_after=idle_after)
    return _STEPS[key]


def _check(oracle, r, clahe):
    c = r["case"]
    for b, it in enumerate(c["items"]):
        n = it["n"]
        at = (c["name"], b, it["kind"])
        pr, fl = r["pri"][b]
        in_kf, _ = R.join(it["lmid"], it["tab_lmid"][it["members"]])
        # the join: flag 2 exactly where the keyframe does not hold the id; else k_prior_frame's flag, and its prior is the designed one
        hp = (it["has_prior"] != 0) & c["use_prior"]
        assert np.array_equal(fl, np.where(in_kf, hp.astype(np.uint8), 2)), at
        sel = in_kf & hp
        assert np.abs(pr[sel] - it["proj"][sel]).max(initial=0) < 1e-3, at
        assert pr[in_kf & ~hp].tobytes() == it["px"][in_kf & ~hp].tobytes(), at
        px, st, p3p = KC.reference(oracle, it, c["use_prior"], clahe, proj=pr, has_prior=fl & 1)
        print("  %s[%d] %-8s n %3d: outside %3d, retried %3d, tracked %3d, rule %d" % (c["name"], b, it["kind"], n, int((st == 4).sum()),
                                                                                      int((st & 2).astype(bool).sum()), int((st & 1).sum()), p3p))
        assert np.array_equal(r["st"][b, :n], st), (at, "status against the oracle")
        assert r["out"][b, :n].tobytes() == px.tobytes(), (at, "out_xy against the oracle")
        assert bool(r["p3p"][b]) == p3p, (at, "p3p_req against the oracle")
        rpx, rst, rp3p = r["route"][b]
        assert r["out"][b, :n].tobytes() == rpx.tobytes() and np.array_equal(r["st"][b, :n], rst) and bool(r["p3p"][b]) == rp3p, (at, "the route")
        out = ~in_kf
        assert np.all(r["st"][b, :n][out] == 4) and r["out"][b, :n][out].tobytes() == it["px"][out].tobytes(), at
    # the item that sat out: its store and its table are as they were
    assert r["idle"]["store"].tobytes() == r["idle_after"]["store"].tobytes() and not r["idle"]["store"].any()
    assert r["idle_after"]["table"]["n"] == 0


@pytest.mark.parametrize("clahe", [False, True], ids=["raw", "clahe"])
@pytest.mark.parametrize("form", ["epi_pose", "mono"])
@pytest.mark.parametrize("name", KC.NAMES)
def test_step_from_the_keyframe_equals_the_oracle_and_the_route(gpu_ctx, oracle, name, form, clahe):
    _check(oracle, _run(gpu_ctx, name, form, clahe), clahe)


def test_resident_step_from_the_keyframe(gpu_ctx, oracle):
    _check(oracle, _run(gpu_ctx, "main", "resident", False), False)


def test_row_kernel_from_the_keyframe(gpu_ctx, oracle):
    r = _run(gpu_ctx, "main", "epi_pose", False, impl="row")
    _check(oracle, r, False)
    w = _run(gpu_ctx, "main", "epi_pose", False)
    assert r["out"].tobytes() == w["out"].tobytes() and r["st"].tobytes() == w["st"].tobytes()


# ---- the resident cycle: keyframe -> 3 frames -> keyframe -> 2 frames ----------------------------------------------------------------
class _Side:
    """the verbs of tests/test_gpu_resident.py's sides on a tracker of BATCH items in the from-keyframe mode"""

    def __init__(self, ctx, which):
        self.ctx, self.which = ctx, which
        self.cal = ov2slam_amd.CameraCalibration(ctx, "pinhole", *TR.K, D=TR.DIST)
        self.t = ov2slam_amd.LockstepTracker(ctx, BATCH, W, H, use_clahe=False, nbmaxkps=N_MAX)
        self.t.setCalibration(self.cal)
        self.t.setTrackFromKeyframe(True)
        self.r = RR.Route(BATCH, N_MAX) if which == "A" else None
        self.cfg = dict(doepipolar=True)

    def frame(self, b):
        return self.r.frames[b] if self.r else self.t.getFrame(b, from_device=False)

    def views(self):
        if self.r:
            v = [RR.frame_bytes(f) for f in self.r.frames]
            return dict(device=v, mirror=v)
        return dict(device=[RR.frame_bytes(self.t.getFrame(b, True)) for b in range(BATCH)],
                    mirror=[RR.frame_bytes(self.t.getFrame(b, False)) for b in range(BATCH)])

    def poses(self):
        return self.r.mir["poses"].copy() if self.r else np.array([self.t.getPose(b) for b in range(BATCH)])

    def states(self):
        return [dict(s) for s in self.r.mir["states"]] if self.r else [self.t.getMotion(b) for b in range(BATCH)]

    def set_pose(self, b, T):
        if self.r:
            self.r.mir["poses"][b] = T
        else:
            self.t.setPose(b, T)

    def update(self, na, ops):
        return self.r.update(na, ops) if self.r else self.t.updateFrame(na, ops)

    def step(self, imgs, a, kw):
        nb = [self.frame(b)["n"] for b in range(len(imgs))]
        res = self.r.step(self.ctx, self.t, imgs, *a, doepipolar=True, **kw) if self.r else self.t.trackMonoResident(imgs, *a, doepipolar=True, **kw)
        return TR._Side.step_record(self, res, nb)

    def ckf(self, na, make_kf, nlmid, nkfid, time, params, state):
        out = CR.empty_out(BATCH, N_MAX)
        if not self.r:
            recs, out = self.t.createKeyframe(na, None, None, None, None, make_kf, nlmid, nkfid, time, params, state, out=out)
            return dict(recs=recs, out=out, state=state.copy(), slot_bytes=self.t.lastSlotBytes())
        recs, out = self.r.create_keyframe(self.ctx, self.t, self.cal, na, make_kf, nlmid, nkfid, time, params, state, out=out)
        # the route of separate calls: the px table by a host sort, the pyramids by the adopt call
        created = np.array([r["action"] == L.OV2_CKF_CREATED for r in recs], np.uint8)
        for b in np.nonzero(created)[0]:
            m = recs[b]["n_kf"]
            o = np.argsort(out["lmid"][b, :m], kind="stable")
            self.t.setKeyframePx(int(b), out["lmid"][b, :m][o], out["px"][b, :m][o])
        self.t.adoptKeyframePyramid(na, created)
        return dict(recs=recs, out=out, state=state.copy(), slot_bytes=None)


def _cycle(ctx, which):
    side = _Side(ctx, which)
    t = side.t
    Kc = tuple(float(v) for v in side.cal.K)
    state = np.full(BATCH, 1e-3, np.float64)
    params = dict(TR.BASE, detector="singlescale")
    fkf = dict(_epi_params(True, False, Kc=Kc)["fkf"], nbmaxkps=TR.BASE["nbmaxkps"])
    nlmid, kfid = np.zeros(BATCH, np.int32), np.zeros(BATCH, np.int32)
    log, stores = [], []

    def note(kind, **kw):
        log.append(dict(kind=kind, views=side.views(), **kw))

    def step(f):
        rng = np.random.default_rng(700 + f)
        seeds = lambda: rng.integers(0, 1 << 63, BATCH).astype(np.uint64) * np.uint64(2) + np.uint64(1)
        a = (_params(pose.LMEDS, False, Kc), dict(_epi_params(True, False, Kc=Kc), fkf=fkf), np.zeros(BATCH, np.uint8), seeds(),
             np.full(BATCH, 3, np.int32), seeds(), np.full(BATCH, 10.0 + f * TR.DT), (kfid + 1).astype(np.int32))
        note("step", f=f, na=NA, **side.step(TR._imgs(f, NA), a, dict(localba_is_on=np.zeros(BATCH, np.uint8), dop3p=False, n_rows=0)))
        for b in range(NA):
            side.set_pose(b, TR._truth(b)[f])

    def ckf(f, make_kf):
        ids = (100 * (f + 1) + np.arange(BATCH)).astype(np.int32)
        r = side.ckf(NA, np.array(make_kf, np.uint8), nlmid.copy(), ids, np.full(BATCH, 10.0 + f * TR.DT + 0.01), params, state)
        for b, rec in enumerate(r["recs"]):
            if rec["action"] == L.OV2_CKF_CREATED:
                nlmid[b] += rec["n_new"]
                kfid[b] = ids[b]
        note("ckf", f=f, na=NA, make_kf=list(make_kf), **r)
        stores.append(dict(kf=[t.kf_item(b).download_item() for b in range(BATCH)], cur=[t.cur_item(b).download_item() for b in range(BATCH)],
                           table=[(t.getKeyframePx(b, True), t.getKeyframePx(b, False)) for b in range(BATCH)], recs=r["recs"], out=r["out"]))

    for b in range(NA):
        side.set_pose(b, TR._truth(b)[0])
    step(0)
    ckf(0, [1, 1, 1, 1])
    note("update", f=1, na=NA, recs=side.update(NA, TR._set_ops(side, 1, NA)))
    for f in (1, 2, 3):
        step(f)
    ckf(3, [1, 0, 1, 1])
    for f in (4, 5):
        step(f)
    t.close()
    return log, stores


def test_resident_cycle_equals_the_host_kept_cycle_and_the_store_follows_the_keyframes(gpu_ctx):
    (A, sa), (B, sb) = _cycle(gpu_ctx, "A"), _cycle(gpu_ctx, "B")
    TR._same_log(A, B, "from the keyframe")
    assert all(e["slot_bytes"] == 0 for e in B if e["kind"] in ("step", "ckf"))
    tracked = [int(((e["st"][b, :e["frames"][b]["n_before"]] & 3) == 1).sum()) for e in B if e["kind"] == "step" and e["f"] > 0 for b in range(NA)]
    assert min(tracked) >= 20, tracked                                    # the steps did track: from the keyframe, up to three frames back
    for which, s in (("A", sa), ("B", sb)):
        first, second = s
        for b in range(BATCH):
            at = (which, b)
            made = b < NA
            # k_kfpyr_adopt: the flagged items' whole stride equals the current pyramid's, the others are untouched
            assert (first["kf"][b].tobytes() == first["cur"][b].tobytes()) if made else not first["kf"][b].any(), at
            if b < NA and second["recs"][b]["action"] == L.OV2_CKF_CREATED:
                assert second["kf"][b].tobytes() == second["cur"][b].tobytes() and second["kf"][b].tobytes() != first["kf"][b].tobytes(), at
            else:
                assert second["kf"][b].tobytes() == first["kf"][b].tobytes(), at
            # the px table: perm / px of create_keyframe's own outputs, on the device and in the mirror
            for k, s_ in enumerate((first, second)):
                dev, mir = s_["table"][b]
                assert dev["n"] == mir["n"] and dev["lmid"].tobytes() == mir["lmid"].tobytes() and dev["px"].tobytes() == mir["px"].tobytes(), at
                if b < NA and s_["recs"][b]["action"] == L.OV2_CKF_CREATED:
                    m = s_["recs"][b]["n_kf"]
                    o = np.argsort(s_["out"]["lmid"][b, :m], kind="stable")
                    assert dev["n"] == m and np.array_equal(dev["lmid"], s_["out"]["lmid"][b, :m][o]), at
                    assert dev["px"].tobytes() == s_["out"]["px"][b, :m][o].tobytes(), at
                elif k == 1:
                    assert dev["lmid"].tobytes() == first["table"][b][0]["lmid"].tobytes() and dev["px"].tobytes() == first["table"][b][0]["px"].tobytes(), at
    assert second["recs"][1]["action"] == L.OV2_CKF_NOT_REQUESTED and sum(r["action"] == L.OV2_CKF_CREATED for r in second["recs"]) == 3
    assert sb[0]["kf"][0].tobytes() == sa[0]["kf"][0].tobytes() and sb[1]["kf"][2].tobytes() == sa[1]["kf"][2].tobytes()


def test_ids_a_temporal_keyframe_took_out_of_the_keyframe_come_out_with_status_4(gpu_ctx):
    """ov2_btracker_temporal_keyframe compacts the resident keyframe's id list on REMOVE_OBS and leaves the px table alone (a snapshot
    that is only looked up by id): in the step that follows exactly the removed ids are outside the keyframe.  The script and the
    verbs of tests/test_gpu_temporalkf.py (mono, pinhole: keyframe 1 removes observations on three items), with the mode on."""
    from tests import temporalkf_ref as TK
    from tests import test_gpu_temporalkf as TT
    s = TT._Side(gpu_ctx, "mono-pinhole", "B", "one")
    t, items, B = s.t, s.S["items"], s.B
    t.setTrackFromKeyframe(True)
    for b in range(B):
        t.setPose(b, items[b]["poses"][0])
        s.set_frame(b, TK.frame_for(items[b], 0, s.known[b]))
    s.step([p[0] for p in s.imgs], 0, "first_frame")
    for k in range(2):
        for b in range(B):
            t.setPose(b, items[b]["poses"][k])
            s.set_frame(b, TK.frame_for(items[b], k, s.known[b]))
        s.ckf(k, "ckf%d" % k)
        tab = [t.getKeyframePx(b, True) for b in range(B)]
        e = s.tkf([1] * B, "kf%d" % k)
    frames = [t.getFrame(b, False) for b in range(B)]
    removed = [(e["out"]["tri_status"][b, :frames[b]["n"]] & L.OV2_TRI_REMOVE_OBS) != 0 for b in range(B)]
    assert sum(int(r.any()) for r in removed) >= 3, [int(r.sum()) for r in removed]
    for b in range(B):
        now = t.getKeyframePx(b, True)
        assert now["n"] == tab[b]["n"] == frames[b]["n"] and now["lmid"].tobytes() == tab[b]["lmid"].tobytes() and now["px"].tobytes() == tab[b]["px"].tobytes()
        assert t.kf_item(b).download_item().tobytes() == t.cur_item(b).download_item().tobytes()
    step = s.step([p[0] for p in s.imgs], 2, "step1")
    for b in range(B):
        n = frames[b]["n"]
        st = step["st"][b, :n]
        assert np.array_equal(st == 4, removed[b]) and not ((st & 4) != 0)[~removed[b]].any(), (b, st, removed[b])
        assert step["out"][b, :n][removed[b]].tobytes() == frames[b]["px"][:n][removed[b]].tobytes(), b
        assert ((st & 3) == 1).sum() >= 0.5 * (~removed[b]).sum(), (b, st)
    s.close()


# ---- mode off after on; refusals -----------------------------------------------------------------------------------------------------
def test_mode_off_after_on_equals_a_tracker_that_never_had_it(gpu_ctx):
    c = KC.case("main")
    items = c["items"]
    res = []
    for toggled in (False, True):
        t = _tracker(gpu_ctx, on=False)
        if toggled:
            t.setTrackFromKeyframe(True)
            t.setTrackFromKeyframe(False)
        empty = _slots([dict(n=0, px=np.zeros((0, 2)), lmid=np.zeros(0), is3d=np.zeros(0), wpt=np.zeros((0, 3)))] * NA)
        _step(t, "epi_pose", [it["kf_img"] for it in items], empty, f=0)
        out, st, p3p = _step(t, "epi_pose", [it["cur_img"] for it in items], _slots(items))
        res.append((out.tobytes(), st.tobytes(), p3p.tobytes(), [tuple(x.tobytes() for x in t.lastPriors(b, it["n"])) for b, it in enumerate(items)]))
        assert not (st & 4).any()
        t.close()
    assert res[0] == res[1]


def test_a_keyframe_replaced_with_the_mode_off_voids_the_adoption(gpu_ctx):
    """on -> off -> a keyframe set or created -> on: the store holds the pyramid of the keyframe before, so the step refuses the item
    until a pyramid is adopted again; the items whose keyframe stayed go on"""
    c = KC.case("main")
    items = c["items"]
    t, cal = _tracker(gpu_ctx), _cal(gpu_ctx)
    _install(t, cal, items, "epi_pose")
    t.setTrackFromKeyframe(False)
    it = items[0]
    m = it["members"]
    unpx, bv = cal.computeKeypoints(it["tab_px"][m])
    t.setKeyframe(0, it["tab_lmid"][m], unpx, bv, I7)
    t.setTrackFromKeyframe(True)
    imgs = [x["cur_img"] for x in items]
    _refused(_step, t, "epi_pose", imgs, _slots(items), c["use_prior"])
    t.adoptKeyframePyramid(1, [1])
    out, st, p3p = _step(t, "epi_pose", imgs, _slots(items), c["use_prior"])
    good = _run(gpu_ctx, "main", "epi_pose", False)
    assert out.tobytes() == good["out"].tobytes() and st.tobytes() == good["st"].tobytes()
    t.close()


def _refused(fn, *a, **kw):
    with pytest.raises(ov2slam_amd.Ov2Error) as e:
        fn(*a, **kw)
    assert e.value.code == L.OV2_EINVAL, e.value


def test_refusals_enqueue_nothing_and_leave_the_state(gpu_ctx):
    c = KC.case("main")
    items = c["items"]
    cal = _cal(gpu_ctx)
    fresh = _tracker(gpu_ctx, on=False)
    _refused(fresh.adoptKeyframePyramid, NA, np.ones(NA, np.uint8))       # no store yet
    _refused(fresh.setKeyframePx, 0, [1, 2], np.zeros((2, 2)))
    assert fresh.kf_item(0) is None
    fresh.close()
    t = _tracker(gpu_ctx)
    a = _slots(items)
    imgs0, imgs1 = [it["kf_img"] for it in items], [it["cur_img"] for it in items]
    I = np.tile(I7, (BATCH, 1))
    frames = lambda: t.lib.ov2_btracker_frames(t.h_trk)
    # the forms without lmid
    zero = np.zeros((BATCH, N_MAX, 2), np.float32)
    _refused(t.trackFrame, imgs0, zero, zero, np.zeros((BATCH, N_MAX), np.uint8), np.zeros(NA, np.int32))
    _refused(t.trackFrameMap, imgs0, a["px"], a["wpt"], a["is3d"], I, np.zeros(NA, np.int32))
    _refused(t.trackFramePose, imgs0, a["px"], a["wpt"], a["is3d"], I, np.zeros(NA, np.int32), _params(pose.LMEDS, True, KC.K), I,
             np.zeros(BATCH, np.uint8), np.arange(1, 2 * BATCH, 2).astype(np.uint64))
    assert frames() == 0
    empty = _slots([dict(n=0, px=np.zeros((0, 2)), lmid=np.zeros(0), is3d=np.zeros(0), wpt=np.zeros((0, 3)))] * NA)
    _step(t, "epi_pose", imgs0, empty, f=0)
    # keypoints, but no adopted pyramid
    _refused(_step, t, "epi_pose", imgs1, a)
    assert frames() == 1
    # the px table: unsorted, repeated, not finite, too long; the table stays
    it = items[0]
    t.setKeyframePx(0, it["tab_lmid"], it["tab_px"])
    before = t.getKeyframePx(0, True)
    _refused(t.setKeyframePx, 0, it["tab_lmid"][::-1], it["tab_px"])
    _refused(t.setKeyframePx, 0, [3, 3], np.zeros((2, 2)))
    _refused(t.setKeyframePx, 0, [3, 4], np.array([[1.0, np.nan], [0, 0]]))
    _refused(t.setKeyframePx, 0, np.arange(N_MAX + 1), np.zeros((N_MAX + 1, 2)))
    _refused(t.setKeyframePx, BATCH, [1], np.zeros((1, 2)))
    for dev in (True, False):
        after = t.getKeyframePx(0, dev)
        assert after["n"] == before["n"] and after["lmid"].tobytes() == before["lmid"].tobytes() and after["px"].tobytes() == before["px"].tobytes()
    # the refused step left the tracker usable: the keyframes installed, the same frames pass, and equal a tracker that was never refused
    for b, it in enumerate(items):
        m = it["members"]
        unpx, bv = cal.computeKeypoints(it["tab_px"][m]) if m.any() else (np.zeros((0, 2), np.float32), np.zeros((0, 3)))
        t.setKeyframe(b, it["tab_lmid"][m], unpx, bv, I7)
        t.setKeyframePx(b, it["tab_lmid"], it["tab_px"])
    t.adoptKeyframePyramid(NA, np.ones(NA, np.uint8))
    # toggling, and the store's calls, while a step is open
    pp, ep = _params(pose.LMEDS, True, KC.K), _epi_params(False, True, Kc=KC.K)
    seeds = np.arange(1, 2 * BATCH, 2).astype(np.uint64)
    t.trackFrameEpiPoseBegin(imgs1, a["px"], a["wpt"], a["is3d"], I, a["n"], pp, ep, I, np.zeros(BATCH, np.uint8), seeds, a["lmid"],
                             np.full(BATCH, 3, np.int32), seeds)
    _refused(t.setTrackFromKeyframe, False)
    _refused(t.setTrackFromKeyframe, True)
    _refused(t.adoptKeyframePyramid, NA, np.ones(NA, np.uint8))
    _refused(t.setKeyframePx, 0, [1], np.zeros((1, 2)))
    _refused(t.getKeyframePx, 0)
    out, st, p3p = t.trackFrameEpiPoseEnd()[:3]
    good = _run(gpu_ctx, "main", "epi_pose", False)
    assert out.tobytes() == good["out"].tobytes() and st.tobytes() == good["st"].tobytes() and np.array_equal(p3p, good["p3p"])
    t.close()
