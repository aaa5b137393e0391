"""Step time of the lock-step tracker on the RESIDENT frame (ov2_btracker_track_mono_resident, ov2_btracker_create_keyframe with
px_h == NULL) against the forms that take the frame from the host, S sequences of 752 x 480 with 308 slots:

    python tools/resident_step_time.py [S] [steps] [rounds] [--forms host,host_compact,resident,ckf_host,ckf_resident] [--out FILE]

The method of tools/trackmono_step_time.py: the frames sit in the tracker's pinned staging sets, every argument is prepared outside
the timed region, every call is timed on its own and ends in its host synchronisation, the forms alternate call by call in one
process, and the median and the quartiles of all timed calls are reported.
  host          ov2_btracker_track_mono on arrays prepared beforehand (308 keypoints an item, 70 % of them 3-D)
  host_compact  the same plus what a caller of that form does before its next call: the next frame compacted on the host with numpy by
                k_mono_pack's rule (one stable argsort of the keep mask over the batch, five take_along_axis)
  resident      ov2_btracker_track_mono_resident; the same frame is installed with ov2_btracker_set_frame per item before each step,
                OUTSIDE the timed region (the step replaces it)
  ckf_host      ov2_btracker_create_keyframe on host arrays: 154 keypoints an item, every item flagged, single scale, BRIEF on
  ckf_resident  the same call on the resident frame (installed before each call, outside the timed region)
Keyframes and poses are set before each step outside the timed region, as tools/trackmono_step_time.py does.
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
            per_c.append((k, wpt, is3d, _invert(T), lmid, kf_lmid, kf_unpx, kf_bv, kf_Twc))
        names = ("kps", "wpt", "is3d", "Twc", "lmid", "kf_lmid", "kf_unpx", "kf_bv", "kf_Twc")
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
    forms = ["host", "host_compact", "resident", "ckf_host", "ckf_resident"]
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

    clock = [10.0]
    nxt = {}

    def step(form, f):
        """-> ms of the timed region"""
        which = f % 3
        kd = kinds[which]
        prepare(which, N if form == "resident" else None)
        clock[0] += 0.05
        tm[:] = clock[0]
        if form == "resident":
            t0 = time.perf_counter()
            L.check(lib.ov2_btracker_track_mono_resident(bt.h_trk, S, ptrs[which], stride, 1, C.byref(mp), C.byref(MIR[which]), vp(out), vp(st), vp(p3p),
                                                         ER, R, MR, FR))
            return (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        L.check(lib.ov2_btracker_track_mono(bt.h_trk, S, ptrs[which], stride, vp(kd["kps"]), vp(kd["wpt"]), vp(kd["is3d"]), vp(n), 1, C.byref(mp),
                                            C.byref(MI[which]), vp(out), vp(st), vp(p3p), ER, R, MR))
        if form == "host_compact":
            # the next frame on the host by k_mono_pack's rule, in slot order
            act = np.array([R[b].action for b in range(S)])
            keep = ((st & 3) == 1) & (e_removed == 0) & (removed == 0)
            keep[(act == L.OV2_POSE_P3P_RESET) | (act == L.OV2_POSE_PNP_RESET)] = False
            order = np.argsort(~keep, axis=1, kind="stable")
            nxt["n"] = keep.sum(1).astype(np.int32)
            nxt["kps"] = np.take_along_axis(out, order[:, :, None], 1)
            nxt["lmid"] = np.take_along_axis(kd["lmid"], order, 1)
            nxt["is3d"] = np.take_along_axis(kd["is3d"], order, 1)
            nxt["wpt"] = np.take_along_axis(kd["wpt"], order[:, :, None], 1)
        return (time.perf_counter() - t0) * 1e3

    def ckf(form):
        quality[:] = 1e-3
        resident = form == "ckf_resident"
        if resident:
            kd = kinds[0]
            for b in range(S):
                L.check(lib.ov2_btracker_set_frame(bt.h_trk, b, NKF, vp(kd["kps"][b]), vp(kd["lmid"][b]), vp(kd["is3d"][b]), vp(kd["wpt"][b])))
        t0 = time.perf_counter()
        L.check(lib.ov2_btracker_create_keyframe(bt.h_trk, S, C.byref(cp), C.byref(CIR if resident else CI), CR, vp(o_px), vp(o_lm), vp(o_un), vp(o_bv),
                                                 vp(o_desc), vp(o_val), vp(o_col)))
        return (time.perf_counter() - t0) * 1e3

    f = 0
    for _ in range(3):                                              # the first frame and two warm-up steps
        step("host", f); f += 1
    times = {form: [] for form in forms}
    rounds = {form: [] for form in forms}
    slot_bytes = {}
    v = C.c_size_t()
    for _ in range(ROUNDS):
        cur = {form: [] for form in forms}
        for _ in range(K):
            for form in forms:                                      # the forms alternate call by call
                if form.startswith("ckf"):
                    cur[form].append(ckf(form))
                else:
                    cur[form].append(step(form, f)); f += 1
                L.check(lib.ov2_btracker_last_slot_bytes(bt.h_trk, C.byref(v)))
                slot_bytes[form] = int(v.value)
        for form in forms:
            times[form] += cur[form]
            rounds[form].append(float(np.median(cur[form])))
    res = dict(tool="resident_step_time", sequences=S, keypoints=N, keyframe_call_keypoints=NKF, steps=K, rounds=ROUNDS, forms={}, slot_bytes=slot_bytes)
    for form in forms:
        t = np.array(times[form])
        res["forms"][form] = dict(median_ms=float(np.median(t)), q25_ms=float(np.percentile(t, 25)), q75_ms=float(np.percentile(t, 75)),
                                  round_medians_ms=rounds[form])
    res["last"] = dict(tracked=float(((st & 3) == 1).mean()), created=int(sum(CR[b].action == L.OV2_CKF_CREATED for b in range(S))),
                       n_kf=int(CR[0].n_kf))
    line = json.dumps(res)
    print(line)
    if OUT:
        with open(OUT, "a") as fh:
            fh.write(line + "\n")
    bt.close(); ctx.close()


if __name__ == "__main__":
    main()
