"""Step time of the lock-step tracker as trackMono after initialisation in one step (ov2_btracker_track_mono) against the route of
separate calls, S sequences of 752 x 480 with 308 keypoints each, 70 % of them 3-D, against a 308-keypoint keyframe:

    python tools/trackmono_step_time.py [S] [steps] [rounds] [--tree DIR] [--forms f18,route,fused] [--out FILE]

The method of tools/frameepi_step_time.py: the frames sit in the tracker's pinned staging sets, every argument is prepared outside
the timed region, every step is timed on its own and ends in its host synchronisation, the forms alternate step by step in one
process, and the median and the quartiles of all timed steps are reported.  --tree DIR imports the package from another checkout (a
build of the parent commit: only `f18` exists there and only it is timed), so that both builds can be measured in one session.
  f18     ov2_btracker_track_frame_epi_pose with caller-supplied poses: the step this change must not slow down
  route   the route's C calls alone: ov2_motion_apply_batch, the f18 step with that pose, ov2_motion_update_batch and
          ov2_kf_decision_batch on a frame of the step's size prepared beforehand (the host compaction a real route needs is NOT in
          the figure: a lower bound of any route)
  fused   ov2_btracker_track_mono
Every step kind has its own keypoints and keyframe; the keyframes are set before each step OUTSIDE the timed region (a real caller
sets one per new keyframe).  The poses: every kind's true pose is handed over with set_pose before the step (outside the timed region),
so that the model predicts from it -- the step's work does not depend on how good the prediction is beyond the tracking it enables.
Prints one JSON line (and appends it to --out)."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

argv = list(sys.argv[1:])
TREE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONLY, OUT = None, None
for flag in ("--tree", "--forms", "--out"):
    if flag in argv:
        i = argv.index(flag)
        if flag == "--tree":
            TREE = os.path.abspath(argv[i + 1])
        elif flag == "--forms":
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
K = int(argv[1]) if len(argv) > 1 else 30
ROUNDS = int(argv[2]) if len(argv) > 2 else 1
W, H, N, ROWS, ITERS = 752, 480, 308, 200, 100
HAS_MONO = "ov2_btracker_track_mono" in L.SIGNATURES


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
    for v in range(3):
        per_c = []
        for c in range(8):
            k = synth.grid_keypoints(W, H, 35, rng)[:N].astype(np.float32)
            k = np.concatenate([k, k[:N - len(k)]]) if len(k) < N else k
            gt = (seqs[c].flow(k.astype(np.float64), (v + 2) % 3, v) + rng.normal(0, 0.7, (N, 2))).astype(np.float32)
            T = _rand_pose(rng)
            bv = cal.computeKeypoints(gt)[1]
            is3d = (rng.uniform(size=N) < 0.7).astype(np.uint8)
            Pc = np.stack([bv[i] / bv[i][2] * rng.uniform(2, 10) for i in range(N)])
            wpt = np.stack([_inv_act(T, Pc[i]) for i in range(N)])
            Pk = Pc @ Rrel.T + trel
            lmid = (10 + 3 * rng.permutation(N)).astype(np.int32)
            o = np.argsort(lmid)
            kf_lmid, Pko = lmid[o], Pk[o]
            kf_unpx = np.stack([Kc[0] * Pko[:, 0] / Pko[:, 2] + Kc[2], Kc[1] * Pko[:, 1] / Pko[:, 2] + Kc[3]], 1).astype(np.float32)
            kf_bv = Pko / np.linalg.norm(Pko, axis=1)[:, None]
            Rcw = _rot_of(T[3:])
            Rwk = Rcw.T @ Rrel.T
            kf_Twc = np.concatenate([-Rcw.T @ T[:3] - Rwk @ trel, _quat_of(Rwk)])
            bad = rng.permutation(N)[:N // 20]
            lmid[bad] = lmid[np.roll(bad, 1)]
            unpx = np.stack([Kc[0] * Pc[:, 0] / Pc[:, 2] + Kc[2], Kc[1] * Pc[:, 1] / Pc[:, 2] + Kc[3]], 1).astype(np.float32)
            per_c.append((k, wpt, is3d, T, _invert(T), lmid, kf_lmid, kf_unpx, kf_bv, kf_Twc, gt, unpx, bv))
        names = ("kps", "wpt", "is3d", "Tcw", "Twc", "lmid", "kf_lmid", "kf_unpx", "kf_bv", "kf_Twc", "px", "unpx", "bv")
        kinds.append({key: np.ascontiguousarray(np.stack([p[j] for p in per_c])[idx]) for j, key in enumerate(names)})
    n = np.full(S, N, np.int32)
    out = np.zeros((S, N, 2), np.float32); st = np.zeros((S, N), np.uint8); p3p = np.zeros(S, np.int32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    dp, ip = (lambda a: a.ctypes.data_as(C.POINTER(C.c_double))), (lambda a: a.ctypes.data_as(C.POINTER(C.c_int)))
    fp_, u8 = (lambda a: a.ctypes.data_as(C.POINTER(C.c_float))), (lambda a: a.ctypes.data_as(C.POINTER(C.c_uint8)))
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

    def epi_input(Twc):
        e = L.FrameEpiPoseInput()
        e.pose.Twc_h = None if Twc is None else dp(Twc)
        e.pose.scale_h, e.pose.p3p_req_h, e.pose.seed_h = None, u8(req), sp
        return e
    FE = []
    for kd in kinds:
        e = epi_input(kd["Twc"])
        e.lmid_h, e.nbkfs_h, e.epi_seed_h = ip(kd["lmid"]), ip(nbkfs), sp
        FE.append(e)
    R = (L.PoseResult * S)(); ER = (L.EpifilterResult * S)()
    removed, e_removed = np.zeros((S, N), np.uint8), np.zeros((S, N), np.uint8)
    for b in range(S):
        R[b].removed, ER[b].removed = u8(removed[b]), u8(e_removed[b])
    forms = ["f18"]
    if HAS_MONO:
        forms += ["route", "fused"]
        mp = L.TrackMonoParams()
        mp.step, mp.doepipolar = fe, 1
        frame_id, ba = np.arange(S, dtype=np.int32) + 5, np.zeros(S, np.uint8)
        tm = np.zeros(S)
        MI = []
        for kd in kinds:
            mi = L.TrackMonoInput()
            mi.step = epi_input(None)
            mi.step.lmid_h, mi.step.nbkfs_h, mi.step.epi_seed_h = ip(kd["lmid"]), ip(nbkfs), sp
            mi.time_h, mi.frame_id_h, mi.localba_is_on_h = dp(tm), ip(frame_id), u8(ba)
            MI.append(mi)
        MR = (L.TrackMonoResult * S)()
        # the route's own calls: states and poses on the host, the frame checkNewKfReq sees prepared at the step's size
        S_in, S_a, S_u = (L.MotionState * S)(), (L.MotionState * S)(), (L.MotionState * S)()
        for b in range(S):
            S_in[b].prev_time = -1.0
            S_in[b].prevTwc[6] = 1.0
        Tw_o, Tc_o, rs = np.zeros((S, 7)), np.zeros((S, 7)), np.zeros(S, np.uint8)
        kf_Tcw = [np.ascontiguousarray(np.stack([keyframe.se3_inverse(T) for T in kd["kf_Twc"][:8]])[idx]) for kd in kinds]
        KI, KR = [(L.FkfItem * S)() for _ in kinds], (L.KfDecisionResult * S)()
        d3 = [np.ascontiguousarray(kd["is3d"]) for kd in kinds]
        for kd, items, kt, f3 in zip(kinds, KI, kf_Tcw, d3):
            for b in range(S):
                f = items[b]
                f.n_cur, f.cur_lmid, f.cur_px, f.cur_unpx, f.cur_bv, f.cur_is3d = N, ip(kd["lmid"][b]), fp_(kd["px"][b]), fp_(kd["unpx"][b]), dp(kd["bv"][b]), u8(f3[b])
                f.cur_Twc, f.n_kf, f.kf_lmid, f.kf_unpx, f.kf_Tcw = dp(kd["Twc"][b]), N, ip(kd["kf_lmid"][b]), fp_(kd["kf_unpx"][b]), dp(kt[b])
                f.cur_id, f.kf_id, f.cur_time, f.kf_time, f.kf_nb3dkps, f.localba_is_on, f.noccupcells, f.nb3dkps = 5 + b, b, 1.0, 0.5, 200, 0, -1, -1
        FKF = keyframe._as_fkf_params(fkf)
    if ONLY:
        forms = [f for f in forms if f in ONLY]

    def set_keyframes(which, mono):
        kd = kinds[which]
        for b in range(S):
            L.check(lib.ov2_btracker_set_keyframe(bt.h_trk, b, N, vp(kd["kf_lmid"][b]), vp(kd["kf_unpx"][b]), vp(kd["kf_bv"][b]), vp(kd["kf_Twc"][b])))
            if mono:
                L.check(lib.ov2_btracker_set_keyframe_info(bt.h_trk, b, b, 0.5, 200))
                L.check(lib.ov2_btracker_set_pose(bt.h_trk, b, vp(kd["Twc"][b])))

    clock = [10.0]

    def step(form, f):
        """-> ms of the timed region"""
        which = f % 3
        kd = kinds[which]
        set_keyframes(which, form == "fused")
        a = (bt.h_trk, S, ptrs[which], stride, vp(kd["kps"]), vp(kd["wpt"]), vp(kd["is3d"]))
        clock[0] += 0.05
        if form == "fused":
            tm[:] = clock[0]
            t0 = time.perf_counter()
            L.check(lib.ov2_btracker_track_mono(*a, vp(n), 1, C.byref(mp), C.byref(MI[which]), vp(out), vp(st), vp(p3p), ER, R, MR))
            return (time.perf_counter() - t0) * 1e3
        if form == "route":
            tm[:] = clock[0]
            t0 = time.perf_counter()
            L.check(lib.ov2_motion_apply_batch(ctx.h, S, S_in, vp(kd["Twc"]), vp(tm), S_a, vp(Tw_o), vp(Tc_o), vp(rs)))
            L.check(lib.ov2_btracker_track_frame_epi_pose(*a, vp(Tc_o), vp(n), 1, C.byref(fe), C.byref(FE[which]), vp(out), vp(st), vp(p3p), ER, R))
            L.check(lib.ov2_motion_update_batch(ctx.h, S, S_a, vp(Tw_o), vp(tm), S_u))
            L.check(lib.ov2_kf_decision_batch(ctx.h, C.byref(FKF), S, KI[which], KR))
            return (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        L.check(lib.ov2_btracker_track_frame_epi_pose(*a, vp(kd["Tcw"]), vp(n), 1, C.byref(fe), C.byref(FE[which]), vp(out), vp(st), vp(p3p), ER, R))
        return (time.perf_counter() - t0) * 1e3

    f = 0
    for _ in range(3):                                              # the first frame and two warm-up steps
        step(forms[0], f); f += 1
    times = {form: [] for form in forms}
    rounds = {form: [] for form in forms}
    for _ in range(ROUNDS):
        cur = {form: [] for form in forms}
        for _ in range(K):
            for form in forms:                                      # the forms alternate step by step
                cur[form].append(step(form, f)); f += 1
        for form in forms:
            times[form] += cur[form]
            rounds[form].append(float(np.median(cur[form])))
    res = dict(tool="trackmono_step_time", tree=TREE, sequences=S, keypoints=N, steps=K, rounds=ROUNDS, forms={})
    for form in forms:
        t = np.array(times[form])
        res["forms"][form] = dict(median_ms=float(np.median(t)), q25_ms=float(np.percentile(t, 25)), q75_ms=float(np.percentile(t, 75)),
                                  round_medians_ms=rounds[form])
    if "fused" in forms:
        res["last_fused"] = dict(tracked=float(((st & 3) == 1).mean()), decisions=int(sum(MR[b].kf.decision for b in range(S))),
                                 resynced=int(sum(MR[b].resynced for b in range(S))))
    line = json.dumps(res)
    print(line)
    if OUT:
        with open(OUT, "a") as fh:
            fh.write(line + "\n")
    bt.close(); ctx.close()


if __name__ == "__main__":
    main()
