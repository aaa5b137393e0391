"""Step time of the lock-step tracker with epipolar2d2dFiltering and the per-frame pose as separate calls and fused into the step
(ov2_btracker_track_frame_epi_pose), S sequences of 752 x 480 with 308 keypoints each, 70 % of them 3-D, against a 308-keypoint
keyframe:

    python tools/frameepi_step_time.py [S] [steps] [rounds] [--tree DIR] [--forms pose,route,fused] [--out FILE]

--tree DIR imports the package from another checkout (a build of the parent commit: only `pose` exists there and only it is timed), so
that both builds can be measured by the same tool in one session, alternating.  The frames sit in the tracker's pinned staging sets,
every argument is prepared outside the timed region, every step is timed on its own and ends in its host synchronisation.  Forms:
  pose    (a) ov2_btracker_track_frame_pose with dop3p = 1: the step without the filter, which must cost what it cost before
  route   (b) track_frame_map, the frame compacted on the host, ov2_epipolar_filter_batch, the filtered pose set compacted on the host,
              ov2_p3p_draw_samples per item, ov2_compute_pose_batch
  fused   (c) ov2_btracker_track_frame_epi_pose with dop3p = 1
The route's host compaction is numpy here (a C driver would be faster), so its pieces are reported separately: `route_c_calls_ms` is
the three C calls alone, a lower bound of any route; then with the host draws; `route` is the whole step.  Every step kind has its own
keypoints, so the fused form sets the items' keyframes before each step, OUTSIDE the timed region (a real caller sets one per new
keyframe).  Settings as tools/framepose_step_time.py and tools/epifilter_time.py: nmaxiter 5, LMedS with 100 iterations over 200
rows for P3P, 100 iterations over 200 rows for the 5-point search, stereo.  Prints one JSON line (and appends it to --out): per form
the median and the quartiles of all timed steps, the medians of every round, and what the last fused step decided."""
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
HAS_EPI = "ov2_btracker_track_frame_epi_pose" in L.SIGNATURES


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
    # per step kind (the frame enters staging set f % 3 and shows view f % 3): keypoints, the map points whose projection under the
    # predicted pose is the true position (+ noise), and that cloud seen from the keyframe's camera, 0.35 m to the side; one keypoint
    # in twenty carries the id of another (a mismatch the filter removes)
    kinds = []
    idx = np.arange(S) % 8
    Rrel = _rot_of(np.array([0.01, -0.015, 0.005, 1.0]) / np.linalg.norm([0.01, -0.015, 0.005, 1.0]))
    trel = np.array([0.35, 0.05, 0.1])
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
            order = rng.permutation(N)
            lmid = (10 + 3 * order).astype(np.int32)
            o = np.argsort(lmid)
            kf_lmid, Pko = lmid[o], Pk[o]
            kf_unpx = np.stack([Kc[0] * Pko[:, 0] / Pko[:, 2] + Kc[2], Kc[1] * Pko[:, 1] / Pko[:, 2] + Kc[3]], 1).astype(np.float32)
            kf_bv = Pko / np.linalg.norm(Pko, axis=1)[:, None]
            Rcw = _rot_of(T[3:])
            Rwk = Rcw.T @ Rrel.T
            kf_Twc = np.concatenate([-Rcw.T @ T[:3] - Rwk @ trel, _quat_of(Rwk)])
            bad = rng.permutation(N)[:N // 20]
            lmid[bad] = lmid[np.roll(bad, 1)]
            per_c.append((k, wpt, is3d, T, _invert(T), lmid, kf_lmid, kf_unpx, kf_bv, kf_Twc))
        names = ("kps", "wpt", "is3d", "Tcw", "Twc", "lmid", "kf_lmid", "kf_unpx", "kf_bv", "kf_Twc")
        kinds.append({key: np.ascontiguousarray(np.stack([p[j] for p in per_c])[idx]) for j, key in enumerate(names)})
    n = np.full(S, N, np.int32)
    out = np.zeros((S, N, 2), np.float32); st = np.zeros((S, N), np.uint8); p3p = np.zeros(S, np.int32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    dp, ip = (lambda a: a.ctypes.data_as(C.POINTER(C.c_double))), (lambda a: a.ctypes.data_as(C.POINTER(C.c_int)))
    fp_, u8 = (lambda a: a.ctypes.data_as(C.POINTER(C.c_float))), (lambda a: a.ctypes.data_as(C.POINTER(C.c_uint8)))
    stride = bt.stride
    params = dict(pnp=dict(nmaxiter=5, chi2th=5.9915, use_robust=True, apply_l2_after_robust=True, K=np.array(Kc)),
                  p3p=dict(mode=pose.LMEDS, max_iterations=ITERS, threshold=pose.threshold(3.0, Kc[0], Kc[1])), mono=False)
    PP = pose._as_pose_params(params)
    fp = L.FramePoseParams()
    fp.pose, fp.dop3p, fp.n_rows = PP, 1, ROWS
    req = np.zeros(S, np.uint8); seed = np.arange(S, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(1)
    FI = []
    for kd in kinds:
        fi = L.FramePoseInput()
        fi.Twc_h = dp(kd["Twc"]); fi.scale_h = None
        fi.p3p_req_h = u8(req); fi.seed_h = seed.ctypes.data_as(C.POINTER(C.c_ulonglong))
        FI.append(fi)
    R = (L.PoseResult * S)()
    removed = np.zeros((S, N), np.uint8)
    for b in range(S):
        R[b].removed = u8(removed[b])
    forms = ["pose"]
    pieces = []
    if HAS_EPI:
        forms += ["route", "fused"]
        EP = keyframe._as_epifilter_params(dict(fkf=dict(K=Kc, ncellsize=35, nbwcells=22, nbhcells=14, nbmaxkps=N, finit_parallax=20.0, stereo=True),
                                                max_iterations=ITERS, threshold=pose.epipolar_threshold(3.0, Kc[0], Kc[1]), fransac_err=3.0,
                                                mono=False, n_rows=ROWS))
        fe = L.FrameEpiPoseParams()
        fe.pose, fe.epi = fp, EP
        nbkfs = np.full(S, 3, np.int32)
        FE = []
        for kd, fi in zip(kinds, FI):
            e = L.FrameEpiPoseInput()
            e.pose = fi
            e.lmid_h, e.nbkfs_h, e.epi_seed_h = ip(kd["lmid"]), ip(nbkfs), seed.ctypes.data_as(C.POINTER(C.c_ulonglong))
            FE.append(e)
        ER = (L.EpifilterResult * S)()
        e_removed = np.zeros((S, N), np.uint8)
        for b in range(S):
            ER[b].removed = u8(e_removed[b])
        # the route's packed arrays at capacity, and its items / problems pointing into them
        c_lmid, c_px, c_un, c_bv, c_3d = np.zeros((S, N), np.int32), np.zeros((S, N, 2), np.float32), np.zeros((S, N, 2), np.float32), np.zeros((S, N, 3)), np.zeros((S, N), np.uint8)
        r_rm = np.zeros((S, N), np.uint8)
        kf_Tcw = [np.ascontiguousarray(np.stack([keyframe.se3_inverse(T) for T in kd["kf_Twc"][:8]])[idx]) for kd in kinds]
        p_unpx, p_wpt, p_bv = np.zeros((S, N, 2)), np.zeros((S, N, 3)), np.zeros((S, N, 3))
        p_sc, p_tab, p_rm = np.zeros((S, N), np.int32), np.zeros((S, ROWS, 4), np.int32), np.zeros((S, N), np.uint8)
        unpx_h, bv_h = np.zeros((S, N, 2), np.float32), np.zeros((S, N, 3))
        EI, ERr = (L.EpifilterItem * S)(), (L.EpifilterResult * S)()
        PB, RB = (L.PoseProblem * S)(), (L.PoseResult * S)()
        for b in range(S):
            f = EI[b].fkf
            f.cur_lmid, f.cur_px, f.cur_unpx, f.cur_bv, f.cur_is3d = ip(c_lmid[b]), fp_(c_px[b]), fp_(c_un[b]), dp(c_bv[b]), u8(c_3d[b])
            f.n_kf, f.noccupcells, f.nb3dkps = N, -1, -1
            EI[b].nbkfs, EI[b].seed = 3, int(seed[b])
            ERr[b].removed = u8(r_rm[b])
            PB[b].unpx, PB[b].wpt, PB[b].bv, PB[b].scale, PB[b].samples = dp(p_unpx[b]), dp(p_wpt[b]), dp(p_bv[b]), ip(p_sc[b]), ip(p_tab[b])
            RB[b].removed = u8(p_rm[b])

    def set_keyframes(which):
        kd = kinds[which]
        for b in range(S):
            L.check(lib.ov2_btracker_set_keyframe(bt.h_trk, b, N, vp(kd["kf_lmid"][b]), vp(kd["kf_unpx"][b]), vp(kd["kf_bv"][b]), vp(kd["kf_Twc"][b])))

    def step(form, f):
        """-> ms of the timed region"""
        which = f % 3
        kd = kinds[which]
        a = (bt.h_trk, S, ptrs[which], stride, vp(kd["kps"]), vp(kd["wpt"]), vp(kd["is3d"]), vp(kd["Tcw"]), vp(n), 1)
        if form == "fused":
            set_keyframes(which)
            t0 = time.perf_counter()
            L.check(lib.ov2_btracker_track_frame_epi_pose(*a, C.byref(fe), C.byref(FE[which]), vp(out), vp(st), vp(p3p), ER, R))
            return (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        if form == "pose":
            L.check(lib.ov2_btracker_track_frame_pose(*a, C.byref(fp), C.byref(FI[which]), vp(out), vp(st), vp(p3p), R))
            return (time.perf_counter() - t0) * 1e3
        L.check(lib.ov2_btracker_track_frame_map(*a, vp(out), vp(st), vp(p3p)))
        t1 = time.perf_counter()
        for b in range(S):                                        # the step's unpx / bv (C calls; part of any route)
            L.check(lib.ov2_btracker_last_keypoints(bt.h_trk, b, N, vp(unpx_h[b]), vp(bv_h[b])))
        mask = (st & 3) == 1
        nc = mask.sum(1).astype(np.int32)
        rank = (np.cumsum(mask, 1) - 1)
        rows = np.nonzero(mask)[0]
        c_lmid[rows, rank[mask]] = kd["lmid"][mask]; c_px[rows, rank[mask]] = out[mask]; c_un[rows, rank[mask]] = unpx_h[mask]
        c_bv[rows, rank[mask]] = bv_h[mask]; c_3d[rows, rank[mask]] = kd["is3d"][mask]
        for b in range(S):
            f_ = EI[b].fkf
            f_.n_cur, f_.cur_Twc, f_.kf_lmid, f_.kf_unpx, f_.kf_Tcw = int(nc[b]), dp(kd["Twc"][b]), ip(kd["kf_lmid"][b]), fp_(kd["kf_unpx"][b]), dp(kf_Tcw[which][b])
            EI[b].kf_bv, EI[b].kf_Twc = dp(kd["kf_bv"][b]), dp(kd["kf_Twc"][b])
        t2 = time.perf_counter()
        L.check(lib.ov2_epipolar_filter_batch(ctx.h, C.byref(EP), S, EI, ERr))
        t3 = time.perf_counter()
        gone = np.zeros((S, N), bool)
        gone[mask] = r_rm[rows, rank[mask]] != 0
        mask2 = mask & (kd["is3d"] != 0) & ~gone
        m = mask2.sum(1).astype(np.int32)
        rows2, rank2 = np.nonzero(mask2)[0], (np.cumsum(mask2, 1) - 1)[mask2]
        p_unpx[rows2, rank2] = unpx_h[mask2]; p_wpt[rows2, rank2] = kd["wpt"][mask2]; p_bv[rows2, rank2] = bv_h[mask2]
        for b in range(S):
            PB[b].n, PB[b].Twc, PB[b].do_p3p, PB[b].p3p_req = int(m[b]), dp(kd["Twc"][b]), 1, 0
            PB[b].n_rows = ROWS if m[b] >= 4 else 0
        t4 = time.perf_counter()
        for b in range(S):
            if m[b] >= 4:
                L.check(lib.ov2_p3p_draw_samples(int(seed[b]), int(m[b]), ROWS, ip(p_tab[b])))
        t5 = time.perf_counter()
        L.check(lib.ov2_compute_pose_batch(ctx.h, C.byref(PP), S, PB, RB))
        t6 = time.perf_counter()
        pieces.append(((t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3, (t4 - t3) * 1e3, (t5 - t4) * 1e3, (t6 - t5) * 1e3))
        return (t6 - t0) * 1e3

    if ONLY:
        forms = [k for k in forms if k in ONLY]
    res, rounds = {k: [] for k in forms}, {k: [] for k in forms}
    f = 0
    for _ in range(3):
        step("pose", f); f += 1
    for r in range(ROUNDS):
        for form in forms:
            for _ in range(3):
                step(form, f); f += 1
            if form == "route":
                del pieces[-3:]
            ts = []
            for _ in range(K):
                ts.append(step(form, f)); f += 1
            res[form] += ts
            rounds[form].append(float(np.median(ts)))
    q = lambda v: dict(median=float(np.median(v)), q1=float(np.percentile(v, 25)), q3=float(np.percentile(v, 75)))
    extra = {}
    if pieces:
        a = np.array(pieces)
        names = ("track_frame_map", "host_compaction_frame_python", "epipolar_filter_batch", "host_compaction_pose_python", "draw_samples",
                 "compute_pose_batch")
        extra["route_pieces_ms"] = {k: q(a[:, j]) for j, k in enumerate(names)}
        extra["route_c_calls_ms"] = q(a[:, 0] + a[:, 2] + a[:, 5])
        extra["route_c_calls_and_draws_ms"] = q(a[:, 0] + a[:, 2] + a[:, 4] + a[:, 5])
    if "fused" in forms:
        extra["last_fused_step"] = dict(filtered_share=float(np.mean([ER[b].action == L.OV2_EPIF_FILTERED for b in range(S)])),
                                        removed_ransac_mean=float(np.mean([ER[b].n_removed_ransac for b in range(S)])),
                                        removed_sampson_mean=float(np.mean([ER[b].n_removed_sampson for b in range(S)])),
                                        pose_accepted_share=float(np.mean([R[b].action == L.OV2_POSE_OK for b in range(S)])))
    bt.close(); ctx.close()
    line = json.dumps(dict(tree=os.path.basename(TREE), S=S, steps=K, rounds=ROUNDS, ms={k: q(v) for k, v in res.items()},
                           round_medians_ms=rounds, **extra))
    print(line)
    if OUT:
        with open(OUT, "a") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
