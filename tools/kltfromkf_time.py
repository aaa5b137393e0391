"""Cost of tracking FROM THE KEYFRAME in the lock-step step (ov2_btracker_set_track_from_keyframe: VisualFrontEnd::kltTrackingFromKF),
S sequences of 752 x 480 with 308 slots, 70 % of them 3-D:

    python tools/kltfromkf_time.py [S] [steps] [rounds] [--forms resident,resident_kf,route_kf,ckf,ckf_adopt,adopt,memcpy] [--out FILE]

The method of tools/resident_step_time.py: the frames sit in the tracker's pinned staging sets, every argument is prepared outside
the timed region, every call is timed on its own and ends in its host synchronisation, the forms alternate call by call in one
process (the mode is switched outside the timed region), and the median and the quartiles of all timed calls are reported.
  resident     ov2_btracker_track_mono_resident with the mode off: the step as it was
  resident_kf  the same step with the mode on: k_kf_join and k_track_klt_kf_w in place of k_track_klt_w, the keyframe store as `prev`
  route_kf     what the fused tracking stage replaces, as separate calls: per item ov2_fb_klt on kf_item / cur_item from the joined
               sources, for the 3-D-prior slots (one level, from the projections) and for the rest (full pyramid, from the frame's
               px); the join is done beforehand and no retry is made: only the tracking stage, a LOWER bound of the route
  ckf          ov2_btracker_create_keyframe on the resident frame (154 keypoints an item, every item flagged), mode off
  ckf_adopt    the same call with the mode on: plus k_kfpx_install and k_kfpyr_adopt in the same enqueue
  adopt        ov2_btracker_adopt_keyframe_pyramid alone, every item flagged (upload of the flags, the copy kernel, one synchronisation)
  memcpy       hipMemcpyAsync device to device of the same bytes (one pyramid set's worth) and one synchronisation
The scene: per image content ONE set of 308 scene points with one id each, followed through the three views of the cycle; a frame
carries every point's position in the view before (the track so far), its map points project near the truth in the current view,
and the keyframe is the view whose pyramids were adopted last, its table holding each id's position in that view.  So a step with
the mode on tracks at most two views back.  The table and the adopted pyramids are installed before the timed calls.  Prints one JSON line (and appends it to --out); the line
carries the bytes k_kfpyr_adopt moves, so that a kernel trace of this tool (--forms adopt) can be set against 8 TB/s."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

argv = list(sys.argv[1:])
TREE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONLY, OUT = None, None
for flag in ("--forms", "--out"):
    if flag in argv:
        i = argv.index(flag)
        if flag == "--forms":
            ONLY = argv[i + 1].split(",")
        else:
            OUT = argv[i + 1]
        del argv[i:i + 2]
sys.path.insert(0, TREE)

import ov2slam_amd                                                 # noqa: E402
from ov2slam_amd import _lib as L                                  # noqa: E402
from ov2slam_amd import keyframe, pose                             # noqa: E402
from ov2slam_amd import synth                                      # noqa: E402
from ov2slam_amd.batch import SyntheticSequence                    # noqa: E402
from tests.match_ref import RADTAN4, EUROC, _inv_act, _rand_pose   # noqa: E402

S = int(argv[0]) if len(argv) > 0 else 4096
K = int(argv[1]) if len(argv) > 1 else 16
ROUNDS = int(argv[2]) if len(argv) > 2 else 1
W, H, N, ROWS, ITERS, NKF = 752, 480, 308, 200, 100, 154


def _invert(T):
    x, y, z, w = T[3:]
    return np.concatenate([_inv_act(T, (0.0, 0.0, 0.0)), [-x, -y, -z, w]])


def _rot_of(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _quat_of(R):
    w = np.sqrt(max(0.0, 1 + R[0, 0] + R[1, 1] + R[2, 2])) / 2            # (small rotations only: w is far from 0)
    return np.array([(R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w), w])


def main():
    ctx = ov2slam_amd.Context(0)
    lib = ctx.lib
    Kc = EUROC["K"]
    cal = ov2slam_amd.CameraCalibration(ctx, "pinhole", *Kc, D=RADTAN4)
    bt = ov2slam_amd.LockstepTracker(ctx, S, W, H, nbmaxkps=N)
    bt.setCalibration(cal)
    rng = np.random.default_rng(5)
    seqs = [SyntheticSequence("s%d" % c, 3, 100 + c, n_views=3) for c in range(8)]      # 8 image contents, three views each
    for which in range(3):
        for b in range(S):
            bt.image_buffers[which][b][:, :W] = seqs[b % 8].views[which]
    ptrs = [(C.c_void_p * S)(*[bt.image_buffers[which][b].ctypes.data for b in range(S)]) for which in range(3)]
    kinds, idx = [], np.arange(S) % 8
    q = np.array([0.01, -0.015, 0.005, 1.0])
    Rrel, trel = _rot_of(q / np.linalg.norm(q)), np.array([0.35, 0.05, 0.1])
    # ONE set of scene points per image content, with one id each, followed through the three views: slot i of every frame and
    # id lmid[i] of every keyframe are the same physical point, pos[c][v][i] is where it lies in view v
    p0, ids, d3, pos = [], [], [], []
    for c in range(8):
        k = synth.grid_keypoints(W, H, 35, rng)[:N].astype(np.float64)
        k = np.concatenate([k, k[:N - len(k)] + 7.0]) if len(k) < N else k
        p0.append(k); ids.append((10 + 3 * rng.permutation(N)).astype(np.int32)); d3.append((rng.uniform(size=N) < 0.7).astype(np.uint8))
        pos.append([k if v == 0 else seqs[c].flow(k, 0, v) for v in range(3)])
    for v in range(3):
        per_c = []
        for c in range(8):
            # the frame carries the track of the view before (a third of a pixel off), the map points project near the truth in view v
            k = (pos[c][(v + 2) % 3] + rng.normal(0, 0.3, (N, 2))).astype(np.float32)
            gt = (pos[c][v] + rng.normal(0, 0.7, (N, 2))).astype(np.float32)
            T = _rand_pose(rng)
            bv = cal.computeKeypoints(gt)[1]
            is3d = d3[c]
            Pc = np.stack([bv[i] / bv[i][2] * rng.uniform(2, 10) for i in range(N)])
            wpt = np.stack([_inv_act(T, Pc[i]) for i in range(N)])
            Pk = Pc @ Rrel.T + trel
            lmid = ids[c]
            o = np.argsort(lmid)
            kf_lmid, Pko = lmid[o], Pk[o]
            kf_unpx = np.stack([Kc[0] * Pko[:, 0] / Pko[:, 2] + Kc[2], Kc[1] * Pko[:, 1] / Pko[:, 2] + Kc[3]], 1).astype(np.float32)
            kf_bv = Pko / np.linalg.norm(Pko, axis=1)[:, None]
            Rcw = _rot_of(T[3:])
            Rwk = Rcw.T @ Rrel.T
            kf_Twc = np.concatenate([-Rcw.T @ T[:3] - Rwk @ trel, _quat_of(Rwk)])
            per_c.append((k, wpt, is3d, _invert(T), lmid, kf_lmid, kf_unpx, kf_bv, kf_Twc, gt, pos[c][v].astype(np.float32)))
        names = ("kps", "wpt", "is3d", "Twc", "lmid", "kf_lmid", "kf_unpx", "kf_bv", "kf_Twc", "proj", "true")
        kinds.append({key: np.ascontiguousarray(np.stack([p[j] for p in per_c])[idx]) for j, key in enumerate(names)})
    n = np.full(S, N, np.int32)
    out = np.zeros((S, N, 2), np.float32); st = np.zeros((S, N), np.uint8); p3p = np.zeros(S, np.int32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    dp, ip = (lambda a: a.ctypes.data_as(C.POINTER(C.c_double))), (lambda a: a.ctypes.data_as(C.POINTER(C.c_int)))
    u8 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint8))
    stride = bt.stride
    params = dict(pnp=dict(nmaxiter=5, chi2th=5.9915, use_robust=True, apply_l2_after_robust=True, K=np.array(Kc)),
                  p3p=dict(mode=pose.LMEDS, max_iterations=ITERS, threshold=pose.threshold(3.0, Kc[0], Kc[1])), mono=False)
    fp = L.FramePoseParams()
    fp.pose, fp.dop3p, fp.n_rows = pose._as_pose_params(params), 1, ROWS
    fkf = dict(K=Kc, ncellsize=35, nbwcells=22, nbhcells=14, nbmaxkps=N, finit_parallax=20.0, stereo=True)
    fe = L.FrameEpiPoseParams()
    fe.pose = fp
    fe.epi = keyframe._as_epifilter_params(dict(fkf=fkf, max_iterations=ITERS, threshold=pose.epipolar_threshold(3.0, Kc[0], Kc[1]),
                                                fransac_err=3.0, mono=False, n_rows=ROWS))
    req = np.zeros(S, np.uint8); seed = np.arange(S, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(1)
    nbkfs = np.full(S, 3, np.int32)
    sp = seed.ctypes.data_as(C.POINTER(C.c_ulonglong))
    R = (L.PoseResult * S)(); ER = (L.EpifilterResult * S)(); MR = (L.TrackMonoResult * S)(); FR = (L.ResidentStepResult * S)()
    removed, e_removed = np.zeros((S, N), np.uint8), np.zeros((S, N), np.uint8)
    for b in range(S):
        R[b].removed, ER[b].removed = u8(removed[b]), u8(e_removed[b])
    mp = L.TrackMonoParams()
    mp.step, mp.doepipolar = fe, 1
    frame_id, ba, tm = np.arange(S, dtype=np.int32) + 5, np.zeros(S, np.uint8), np.zeros(S)
    MI, MIR = [], []
    for kd in kinds:
        for lst, resident in ((MI, False), (MIR, True)):
            mi = L.TrackMonoInput()
            mi.step.pose.Twc_h, mi.step.pose.scale_h, mi.step.pose.p3p_req_h, mi.step.pose.seed_h = None, None, u8(req), sp
            mi.step.lmid_h, mi.step.nbkfs_h, mi.step.epi_seed_h = (None if resident else ip(kd["lmid"])), ip(nbkfs), sp
            mi.time_h, mi.frame_id_h, mi.localba_is_on_h = dp(tm), ip(frame_id), u8(ba)
            lst.append(mi)
    # createKeyframe: 154 keypoints an item (the first half of the step's), every item flagged
    cp, CI, CIR = L.CreateKeyframeParams(), L.CreateKeyframeInput(), L.CreateKeyframeInput()
    cp.ncellsize, cp.nbwcells, cp.nbhcells, cp.nbmaxkps, cp.detector, cp.det_cell = 35, 22, 14, N, L.OV2_CKF_DET_SINGLESCALE, 35
    cp.roi = (C.c_int * 4)(5, 5, W - 10, H - 10)
    cp.mask_mode, cp.do_subpix, cp.use_brief = L.OV2_MASK_AS_EXECUTED, 1, 1
    n_kf, mk, nlmid, nkfid, ktime = np.full(S, NKF, np.int32), np.ones(S, np.uint8), np.full(S, 100000, np.int32), np.arange(S, dtype=np.int32), np.zeros(S)
    quality = np.full(S, 1e-3)
    for ci, resident in ((CI, False), (CIR, True)):
        kd = kinds[0]
        if not resident:
            ci.px_h, ci.lmid_h, ci.is3d_h, ci.n_h = kd["kps"].ctypes.data_as(C.POINTER(C.c_float)), ip(kd["lmid"]), u8(kd["is3d"]), ip(n_kf)
        ci.make_kf_h, ci.nlmid_h, ci.nkfid_h, ci.time_h, ci.Twc_h, ci.quality_inout = u8(mk), ip(nlmid), ip(nkfid), dp(ktime), None, dp(quality)
    CR = (L.CreateKeyframeResult * S)()
    o_px, o_lm, o_un, o_bv = np.zeros((S, N, 2), np.float32), np.zeros((S, N), np.int32), np.zeros((S, N, 2), np.float32), np.zeros((S, N, 3))
    o_desc, o_val, o_col = np.zeros((S, N, 32), np.uint8), np.zeros((S, N), np.uint8), np.zeros((S, N), np.uint8)
    forms = ["resident", "resident_kf", "route_kf", "ckf", "ckf_adopt", "adopt", "memcpy"]
    if ONLY:
        forms = [f for f in forms if f in ONLY]

    def prepare(which, n_frame=None):
        """outside the timed region: the keyframes, their info and the poses; n_frame: install the resident frames too"""
        kd = kinds[which]
        for b in range(S):
            L.check(lib.ov2_btracker_set_keyframe(bt.h_trk, b, N, vp(kd["kf_lmid"][b]), vp(kd["kf_unpx"][b]), vp(kd["kf_bv"][b]), vp(kd["kf_Twc"][b])))
            L.check(lib.ov2_btracker_set_keyframe_info(bt.h_trk, b, b, 0.5, 200))
            L.check(lib.ov2_btracker_set_pose(bt.h_trk, b, vp(kd["Twc"][b])))
            if n_frame is not None:
                L.check(lib.ov2_btracker_set_frame(bt.h_trk, b, n_frame, vp(kd["kps"][b]), vp(kd["lmid"][b]), vp(kd["is3d"][b]), vp(kd["wpt"][b])))

    def kf_mode(on):
        L.check(lib.ov2_btracker_set_track_from_keyframe(bt.h_trk, 1 if on else 0))

    store, armed = [0], [False]

    def install_store(which):
        """the keyframe of every item is view `which`, whose pyramids are the current ones: the px table holds each id's position
        in THAT view, by ascending id, and the current pyramids are adopted"""
        kd = kinds[which]
        for b in range(S):
            o = np.argsort(kd["lmid"][b], kind="stable")
            lm, px = np.ascontiguousarray(kd["lmid"][b][o]), np.ascontiguousarray(kd["true"][b][o])
            L.check(lib.ov2_btracker_set_keyframe_px(bt.h_trk, b, N, vp(lm), vp(px)))
        L.check(lib.ov2_btracker_adopt_keyframe_pyramid(bt.h_trk, S, vp(mk)))
        store[0] = which
        armed[0] = True

    clock = [10.0]
    pyr_bytes = int(lib.ov2_pyr_item_bytes(C.c_void_p(lib.ov2_btracker_cur_item(bt.h_trk, 0))))
    ft = ov2slam_amd.FeatureTracker(ctx, 30, 0.01)
    hip = C.CDLL("libamdhip64.so")                                   # the runtime the library itself is linked against
    d_src, d_dst = C.c_void_p(), C.c_void_p()
    for p in (d_src, d_dst):
        assert hip.hipMalloc(C.byref(p), C.c_size_t(S * pyr_bytes)) == 0
        assert hip.hipMemset(p, 0, C.c_size_t(S * pyr_bytes)) == 0

    def step(form, f):
        """-> ms of the timed region"""
        which = f % 3
        if armed[0]:
            kf_mode(True)                                            # (a keyframe set with the mode off would void the adoption)
        prepare(which, N)
        kf_mode(form == "resident_kf")
        clock[0] += 0.05
        tm[:] = clock[0]
        t0 = time.perf_counter()
        L.check(lib.ov2_btracker_track_mono_resident(bt.h_trk, S, ptrs[which], stride, 1, C.byref(mp), C.byref(MIR[which]), vp(out), vp(st), vp(p3p),
                                                     ER, R, MR, FR))
        return (time.perf_counter() - t0) * 1e3

    def route(f):
        """the tracking stage as separate calls: per item the joined sources (the keyframe's px of each slot's id), then ov2_fb_klt
        between its keyframe's view and its current view on one level from the projections and on the full pyramid from the frame's px"""
        kd, src = kinds[f % 3], kinds[store[0]]["true"]              # (slot i is point i in every view: the join is the identity)
        views = [(bt.kf_item(b), bt.cur_item(b)) for b in range(S)]
        hp = kd["is3d"] != 0
        t0 = time.perf_counter()
        for b in range(S):
            kp, cp = views[b]
            ft.fbKltTracking(kp, cp, 9, 1, 30.0, 0.5, src[b][hp[b]], kd["proj"][b][hp[b]])
            ft.fbKltTracking(kp, cp, 9, 3, 30.0, 0.5, src[b][~hp[b]], kd["kps"][b][~hp[b]])
        return (time.perf_counter() - t0) * 1e3

    def ckf(form):
        quality[:] = 1e-3
        kd = kinds[0]
        for b in range(S):
            L.check(lib.ov2_btracker_set_frame(bt.h_trk, b, NKF, vp(kd["kps"][b]), vp(kd["lmid"][b]), vp(kd["is3d"][b]), vp(kd["wpt"][b])))
        kf_mode(form == "ckf_adopt")
        t0 = time.perf_counter()
        L.check(lib.ov2_btracker_create_keyframe(bt.h_trk, S, C.byref(cp), C.byref(CIR), CR, vp(o_px), vp(o_lm), vp(o_un), vp(o_bv),
                                                 vp(o_desc), vp(o_val), vp(o_col)))
        return (time.perf_counter() - t0) * 1e3

    def adopt():
        t0 = time.perf_counter()
        L.check(lib.ov2_btracker_adopt_keyframe_pyramid(bt.h_trk, S, vp(mk)))
        return (time.perf_counter() - t0) * 1e3

    def memcpy():
        t0 = time.perf_counter()
        assert hip.hipMemcpyAsync(d_dst, d_src, C.c_size_t(S * pyr_bytes), 3, None) == 0          # hipMemcpyDeviceToDevice
        assert hip.hipDeviceSynchronize() == 0
        return (time.perf_counter() - t0) * 1e3

    f = 0
    kf_mode(False)
    for _ in range(3):                                              # the first frame and two warm-up steps
        step("resident", f); f += 1
    kf_mode(True)
    install_store((f - 1) % 3)
    for _ in range(2):                                              # and two of the other mode
        step("resident_kf", f); f += 1
    times = {form: [] for form in forms}
    rounds = {form: [] for form in forms}
    for _ in range(ROUNDS):
        cur = {form: [] for form in forms}
        for _ in range(K):
            for form in forms:                                      # the forms alternate call by call
                if form.startswith("ckf"):
                    cur[form].append(ckf(form))
                    kf_mode(True)
                    install_store((f - 1) % 3)                      # (the keyframe call replaced the store and the resident keyframe)
                elif form == "adopt":
                    cur[form].append(adopt())
                elif form == "memcpy":
                    cur[form].append(memcpy())
                elif form == "route_kf":
                    cur[form].append(route(f - 1))
                else:
                    cur[form].append(step(form, f)); f += 1
        for form in forms:
            times[form] += cur[form]
            rounds[form].append(float(np.median(cur[form])))
    res = dict(tool="kltfromkf_time", sequences=S, keypoints=N, keyframe_call_keypoints=NKF, steps=K, rounds=ROUNDS, forms={},
               pyramid_item_bytes=pyr_bytes, adopt_bytes_read_plus_written=2 * S * pyr_bytes)
    for form in forms:
        t = np.array(times[form])
        res["forms"][form] = dict(median_ms=float(np.median(t)), q25_ms=float(np.percentile(t, 25)), q75_ms=float(np.percentile(t, 75)),
                                  round_medians_ms=rounds[form])
    res["last"] = dict(tracked=float(((st & 3) == 1).mean()), not_in_keyframe=float((st == 4).mean()),
                       created=int(sum(CR[b].action == L.OV2_CKF_CREATED for b in range(S))), n_kf=int(CR[0].n_kf))
    line = json.dumps(res)
    print(line)
    if OUT:
        with open(OUT, "a") as fh:
            fh.write(line + "\n")
    bt.close(); ctx.close()


if __name__ == "__main__":
    main()
