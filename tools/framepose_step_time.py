"""Step time of the lock-step tracker with the per-frame pose as separate calls and fused into the step
(ov2_btracker_track_frame_pose), S sequences of 752 x 480 with 308 keypoints each, 70 % of them 3-D:

    python tools/framepose_step_time.py [S] [steps] [rounds] [--tree DIR] [--forms map,fused,...]

--tree DIR imports the package from another checkout (a build of the parent commit: only `map` exists there and only it is timed), so
that both builds can be measured by the same tool in one session, alternating.  The frames sit in the tracker's pinned staging sets,
every argument is prepared outside the timed region, every step is timed on its own and ends in its host synchronisation.  Forms:
  map         (a) ov2_btracker_track_frame_map
  route       (b) track_frame_map, the pose set compacted on the host, ov2_compute_pose_batch; without P3P
  route+p3p   (b) the same with do_p3p on every item: the host also draws every item's table (ov2_p3p_draw_samples)
  fused       (c) ov2_btracker_track_frame_pose; without P3P
  fused+p3p   (c) with dop3p = 1
The route's host compaction is numpy here (a C driver would be faster), so its pieces are reported separately: `route_c_calls` is
the two C calls alone (track_frame_map + ov2_compute_pose_batch [+ the draws]), a lower bound of any route; `route` is the whole step.
Pose settings as tools/computepose_time.py: nmaxiter 5, LMedS with 100 iterations over 200 rows.  Prints one JSON line: per form the
median ms of every round's steps, and the share of items whose pose was accepted in the last fused step."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

argv = list(sys.argv[1:])
TREE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if "--tree" in argv:
    i = argv.index("--tree")
    TREE = os.path.abspath(argv[i + 1])
    del argv[i:i + 2]
ONLY = None
if "--forms" in argv:                                              # e.g. --forms fused+p3p: time these forms only (a kernel trace of one form)
    i = argv.index("--forms")
    ONLY = argv[i + 1].split(",")
    del argv[i:i + 2]
sys.path.insert(0, TREE)

import ov2slam_amd                                                 # noqa: E402
from ov2slam_amd import _lib as L                                  # noqa: E402
from ov2slam_amd import pose                                       # noqa: E402
from ov2slam_amd import synth                                      # noqa: E402
from ov2slam_amd.batch import SyntheticSequence                    # noqa: E402
from tests.match_ref import RADTAN4, EUROC, _inv_act, _rand_pose   # noqa: E402

S = int(argv[0]) if len(argv) > 0 else 4096
K = int(argv[1]) if len(argv) > 1 else 30
ROUNDS = int(argv[2]) if len(argv) > 2 else 3
W, H, N, ROWS, ITERS = 752, 480, 308, 200, 100
HAS_POSE = "ov2_btracker_track_frame_pose" in L.SIGNATURES


def _invert(T):
    x, y, z, w = T[3:]
    return np.concatenate([_inv_act(T, (0.0, 0.0, 0.0)), [-x, -y, -z, w]])


def main():
    ctx = ov2slam_amd.Context(0)
    lib = ctx.lib
    cal = ov2slam_amd.CameraCalibration(ctx, "pinhole", *EUROC["K"], D=RADTAN4)
    bt = ov2slam_amd.LockstepTracker(ctx, S, W, H, nbmaxkps=N)
    bt.setCalibration(cal)
    rng = np.random.default_rng(5)
    seqs = [SyntheticSequence("s%d" % c, 3, 100 + c, n_views=3) for c in range(8)]      # 8 image contents, three views each
    for which in range(3):
        for b in range(S):
            bt.image_buffers[which][b][:, :W] = seqs[b % 8].views[which]
    ptrs = [(C.c_void_p * S)(*[bt.image_buffers[which][b].ctypes.data for b in range(S)]) for which in range(3)]
    # per step kind (the frame enters staging set f % 3 and shows view f % 3): keypoints and the map points whose projection under
    # the predicted pose is the true position (+ noise)
    kinds = []
    idx = np.arange(S) % 8
    for v in range(3):
        per_c = []
        for c in range(8):
            k = synth.grid_keypoints(W, H, 35, rng)[:N].astype(np.float32)
            k = np.concatenate([k, k[:N - len(k)]]) if len(k) < N else k
            gt = (seqs[c].flow(k.astype(np.float64), (v + 2) % 3, v) + rng.normal(0, 0.7, (N, 2))).astype(np.float32)
            T = _rand_pose(rng)
            bv = cal.computeKeypoints(gt)[1]
            is3d = (rng.uniform(size=N) < 0.7).astype(np.uint8)
            wpt = np.stack([_inv_act(T, bv[i] / bv[i][2] * rng.uniform(2, 10)) for i in range(N)])
            per_c.append((k, wpt, is3d, T, _invert(T)))
        kinds.append({key: np.ascontiguousarray(np.stack([p[j] for p in per_c])[idx]) for j, key in enumerate(("kps", "wpt", "is3d", "Tcw", "Twc"))})
    n = np.full(S, N, np.int32)
    out = np.zeros((S, N, 2), np.float32); st = np.zeros((S, N), np.uint8); p3p = np.zeros(S, np.int32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    stride = bt.stride
    forms = ["map"]
    if HAS_POSE:
        forms += ["route", "route+p3p", "fused", "fused+p3p"]
        params = dict(pnp=dict(nmaxiter=5, chi2th=5.9915, use_robust=True, apply_l2_after_robust=True, K=np.array(EUROC["K"])),
                      p3p=dict(mode=pose.LMEDS, max_iterations=ITERS, threshold=pose.threshold(3.0, EUROC["K"][0], EUROC["K"][1])), mono=False)
        PP = pose._as_pose_params(params)
        FP = {}
        for dop3p in (0, 1):
            fp = L.FramePoseParams()
            fp.pose, fp.dop3p, fp.n_rows = PP, dop3p, ROWS
            FP[dop3p] = fp
        req = np.zeros(S, np.uint8); seed = np.arange(S, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(1)
        FI = []
        for kd in kinds:
            fi = L.FramePoseInput()
            fi.Twc_h = kd["Twc"].ctypes.data_as(C.POINTER(C.c_double)); fi.scale_h = None
            fi.p3p_req_h = req.ctypes.data_as(C.POINTER(C.c_uint8)); fi.seed_h = seed.ctypes.data_as(C.POINTER(C.c_ulonglong))
            FI.append(fi)
        R = (L.PoseResult * S)()
        removed = np.zeros((S, N), np.uint8)
        # the route's packed arrays at capacity, and its problems pointing into them (only n and do_p3p change from step to step)
        c_unpx, c_wpt, c_bv = np.zeros((S, N, 2)), np.zeros((S, N, 3)), np.zeros((S, N, 3))
        c_sc, c_tab, c_rm = np.zeros((S, N), np.int32), np.zeros((S, ROWS, 4), np.int32), np.zeros((S, N), np.uint8)
        unpx_h, bv_h = np.zeros((S, N, 2), np.float32), np.zeros((S, N, 3))
        PB, RB = (L.PoseProblem * S)(), (L.PoseResult * S)()
        dp, ip = (lambda a: a.ctypes.data_as(C.POINTER(C.c_double))), (lambda a: a.ctypes.data_as(C.POINTER(C.c_int)))
        for b in range(S):
            R[b].removed = removed[b].ctypes.data_as(C.POINTER(C.c_uint8))
            PB[b].unpx, PB[b].wpt, PB[b].bv, PB[b].scale, PB[b].samples = dp(c_unpx[b]), dp(c_wpt[b]), dp(c_bv[b]), ip(c_sc[b]), ip(c_tab[b])
            RB[b].removed = c_rm[b].ctypes.data_as(C.POINTER(C.c_uint8))
        pieces = {"route": [], "route+p3p": []}

    def step(form, f):
        which = f % 3
        kd = kinds[which]
        if form.startswith("fused"):
            L.check(lib.ov2_btracker_track_frame_pose(bt.h_trk, S, ptrs[which], stride, vp(kd["kps"]), vp(kd["wpt"]), vp(kd["is3d"]), vp(kd["Tcw"]),
                                                      vp(n), 1, C.byref(FP[int(form.endswith("p3p"))]), C.byref(FI[which]), vp(out), vp(st), vp(p3p), R))
            return
        t0 = time.perf_counter()
        L.check(lib.ov2_btracker_track_frame_map(bt.h_trk, S, ptrs[which], stride, vp(kd["kps"]), vp(kd["wpt"]), vp(kd["is3d"]), vp(kd["Tcw"]),
                                                 vp(n), 1, vp(out), vp(st), vp(p3p)))
        if form == "map":
            return
        t1 = time.perf_counter()
        do_p3p = form.endswith("p3p")
        for b in range(S):                                        # the step's unpx / bv (C calls; part of any route)
            L.check(lib.ov2_btracker_last_keypoints(bt.h_trk, b, N, vp(unpx_h[b]), vp(bv_h[b])))
        mask = ((st & 3) == 1) & (kd["is3d"] != 0)
        m = mask.sum(1).astype(np.int32)
        rows, rank = np.nonzero(mask)[0], (np.cumsum(mask, 1) - 1)[mask]
        c_unpx[rows, rank] = unpx_h[mask]; c_wpt[rows, rank] = kd["wpt"][mask]; c_bv[rows, rank] = bv_h[mask]
        for b in range(S):
            PB[b].n, PB[b].Twc, PB[b].do_p3p, PB[b].p3p_req = int(m[b]), dp(kd["Twc"][b]), int(do_p3p), 0
            PB[b].n_rows = ROWS if do_p3p and m[b] >= 4 else 0
        t2 = time.perf_counter()
        if do_p3p:
            for b in range(S):
                if m[b] >= 4:
                    L.check(lib.ov2_p3p_draw_samples(int(seed[b]), int(m[b]), ROWS, ip(c_tab[b])))
        t3 = time.perf_counter()
        L.check(lib.ov2_compute_pose_batch(ctx.h, C.byref(PP), S, PB, RB))
        t4 = time.perf_counter()
        pieces[form].append(((t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3, (t4 - t3) * 1e3))

    if ONLY:
        forms = [k for k in forms if k in ONLY]
    res = {k: [] for k in forms}
    f = 0
    for _ in range(3):
        step("map", f); f += 1
    for r in range(ROUNDS):
        for form in forms:
            for _ in range(3):
                step(form, f); f += 1
            if form in ("route", "route+p3p"):
                del pieces[form][-3:]
            ts = []
            for _ in range(K):
                t = time.perf_counter()
                step(form, f); f += 1
                ts.append((time.perf_counter() - t) * 1e3)
            res[form].append(float(np.median(ts)))
    extra = {}
    if HAS_POSE:
        for form, v in pieces.items():
            if not v:
                continue
            a = np.median(np.array(v), 0)
            extra[form + "_pieces_ms"] = dict(track_frame_map=float(a[0]), host_compaction_python=float(a[1]), draw_samples=float(a[2]),
                                              compute_pose_batch=float(a[3]))
            extra[form + "_c_calls_ms"] = float(a[0] + a[2] + a[3])
        step("fused+p3p", f)
        extra["accepted_share_last_fused_step"] = float(np.mean([R[b].action == L.OV2_POSE_OK for b in range(S)]))
        extra["searched_share_last_fused_step"] = float(np.mean([R[b].ran_p3p for b in range(S)]))
    bt.close(); ctx.close()
    print(json.dumps(dict(tree=os.path.basename(TREE), S=S, steps=K, rounds=ROUNDS, round_medians_ms=res,
                          median_ms={k: float(np.median(v)) for k, v in res.items()},
                          spread_ms={k: float(np.max(v) - np.min(v)) for k, v in res.items()}, **extra)))


if __name__ == "__main__":
    main()
