"""Time of MapManager::createKeyframe for the flagged items of a lock-step batch as one call (ov2_btracker_create_keyframe) against the
C calls of the route it replaces, S sequences of 752 x 480 with 308 slots and 154 tracked keypoints each (one in every second cell of
the 35 px grid), single scale with cell 35, BRIEF on:

    python tools/createkf_time.py [S] [calls] [rounds] [--flag all|fifth] [--out FILE]

The method of tools/frameepi_step_time.py: one process, the forms alternate round by round, every argument is prepared outside the
timed region, every call is timed on its own and ends in its own host synchronisation; the median and the quartiles of all timed
calls are reported.  --flag fifth: one item in five is asked to become a keyframe (the others cost the fused call a skip byte; the
route's detector has no such byte and runs over the batch).  Forms:
  route   the route's C calls alone: ov2_btracker_describe_brief of the frame, ov2_btracker_detect_singlescale,
          ov2_btracker_describe_brief of the new points, ONE ov2_compute_keypoints over every slot of the batch, and
          ov2_btracker_set_keyframe + ov2_btracker_set_keyframe_info per flagged item on arrays of the frame's size prepared beforehand.
          What a real route does on the host in between (occupied cells, appending, ids, the sort by lmid, the colour) is NOT in the
          figure: a lower bound of any route.  `route_pieces_ms` gives the calls one by one.
  fused   ov2_btracker_create_keyframe
The detector's quality is put back to its start before every call, so that every call does the same work.
Prints one JSON line (and appends it to --out)."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

argv = list(sys.argv[1:])
TREE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAG, OUT = "all", None
for flag in ("--flag", "--out"):
    if flag in argv:
        i = argv.index(flag)
        if flag == "--flag":
            FLAG = argv[i + 1]
        else:
            OUT = argv[i + 1]
        del argv[i:i + 2]
sys.path.insert(0, TREE)

import ov2slam_amd                                                 # noqa: E402
from ov2slam_amd import _lib as L                                  # noqa: E402
from ov2slam_amd.batch import SyntheticSequence                    # noqa: E402
from tests.match_ref import RADTAN4, EUROC                         # noqa: E402

S = int(argv[0]) if len(argv) > 0 else 4096
K = int(argv[1]) if len(argv) > 1 else 20
ROUNDS = int(argv[2]) if len(argv) > 2 else 2
W, H, N, CELL = 752, 480, 308, 35
NBW, NBH = (W + CELL - 1) // CELL, (H + CELL - 1) // CELL          # the frame grid: 22 x 14 = 308 cells


def main():
    ctx = ov2slam_amd.Context(0)
    lib = ctx.lib
    Kc = EUROC["K"]
    cal = ov2slam_amd.CameraCalibration(ctx, "pinhole", *Kc, D=RADTAN4)
    bt = ov2slam_amd.LockstepTracker(ctx, S, W, H, nbmaxkps=N)
    bt.setCalibration(cal)
    rng = np.random.default_rng(5)
    seqs = [SyntheticSequence("s%d" % c, 3, 100 + c, n_views=3) for c in range(8)]      # 8 image contents
    for b in range(S):
        bt.image_buffers[0][b][:, :W] = seqs[b % 8].views[0]
    z2 = np.zeros((S, N, 2), np.float32)
    bt.trackFrame([bt.image_buffers[0][b] for b in range(S)], z2, z2, None, np.zeros(S, np.int32))      # the current frame: pyramid and raw
    for b in range(S):
        bt.setPose(b, np.array([0.1 * (b % 7), 0.0, 0.0, 0.0, 0.0, 0.0, 1.0]))
    # 154 tracked keypoints per content: every second cell of the frame grid (a checkerboard), well inside its cell
    cells = [(r, c) for r in range(NBH) for c in range(NBW) if (r + c) % 2 == 0][:N // 2]
    per_c = []
    for c8 in range(8):
        p = np.array([(min(CELL * c + rng.uniform(8, 27), W - 3), min(CELL * r + rng.uniform(8, 27), H - 3)) for r, c in cells], np.float32)
        per_c.append(p)
    n_prev = len(cells)
    px = np.zeros((S, N, 2), np.float32)
    px[:, :n_prev] = np.stack(per_c)[np.arange(S) % 8]
    lmid = np.zeros((S, N), np.int32)
    lmid[:, :n_prev] = np.stack([rng.permutation(1000)[:n_prev] for _ in range(8)])[np.arange(S) % 8]
    is3d = np.zeros((S, N), np.uint8); is3d[:, :n_prev] = rng.uniform(size=(S, n_prev)) < 0.7
    n = np.full(S, n_prev, np.int32)
    mk = np.ones(S, np.uint8) if FLAG == "all" else (np.arange(S) % 5 == 0).astype(np.uint8)
    flagged = np.nonzero(mk)[0]
    nlmid, nkfid, tm = np.full(S, 1000, np.int32), np.arange(S, dtype=np.int32), np.full(S, 12.5)
    quality = np.full(S, 1e-3)
    roi = (C.c_int * 4)(5, 5, W - 10, H - 10)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    # ---- the fused call's arguments
    cp, ci = L.CreateKeyframeParams(), L.CreateKeyframeInput()
    cp.ncellsize, cp.nbwcells, cp.nbhcells, cp.nbmaxkps, cp.detector, cp.det_cell = CELL, NBW, NBH, N, L.OV2_CKF_DET_SINGLESCALE, CELL
    cp.roi, cp.mask_mode, cp.do_subpix, cp.use_brief = roi, 0, 1, 1
    ci.px_h, ci.lmid_h, ci.is3d_h = px.ctypes.data_as(C.POINTER(C.c_float)), lmid.ctypes.data_as(C.POINTER(C.c_int)), is3d.ctypes.data_as(C.POINTER(C.c_uint8))
    ci.n_h, ci.make_kf_h = n.ctypes.data_as(C.POINTER(C.c_int)), mk.ctypes.data_as(C.POINTER(C.c_uint8))
    ci.nlmid_h, ci.nkfid_h, ci.time_h = nlmid.ctypes.data_as(C.POINTER(C.c_int)), nkfid.ctypes.data_as(C.POINTER(C.c_int)), tm.ctypes.data_as(C.POINTER(C.c_double))
    ci.Twc_h, ci.quality_inout, ci.fast_th_inout = None, quality.ctypes.data_as(C.POINTER(C.c_double)), None
    R = (L.CreateKeyframeResult * S)()
    o_px, o_lm, o_un, o_bv = np.zeros((S, N, 2), np.float32), np.zeros((S, N), np.int32), np.zeros((S, N, 2), np.float32), np.zeros((S, N, 3))
    o_desc, o_val, o_col = np.zeros((S, N, 32), np.uint8), np.zeros((S, N), np.uint8), np.zeros((S, N), np.uint8)
    # ---- the route's arguments: results of the detector, the new frame for computeKeypoints, ascending ids and a pose for set_keyframe
    cap = 2 * (W // CELL) * (H // CELL)
    det = np.zeros((S, cap, 2), np.float32); det_n = np.zeros(S, np.int32)
    new_pts = np.zeros((S, N, 2), np.float32); new_n = np.zeros(S, np.int32)
    d0, v0, d1, v1 = np.zeros((S, N, 32), np.uint8), np.zeros((S, N), np.uint8), np.zeros((S, N, 32), np.uint8), np.zeros((S, N), np.uint8)
    frame = px.copy()
    r_un, r_bv = np.zeros((S, N, 2), np.float32), np.zeros((S, N, 3))
    asc = np.arange(N, dtype=np.int32)
    Twc = np.array([0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0])
    Dp = vp(cal.D) if cal.D is not None else None
    pieces = []

    def call(form):
        quality[:] = 1e-3
        t0 = time.perf_counter()
        if form == "fused":
            L.check(lib.ov2_btracker_create_keyframe(bt.h_trk, S, C.byref(cp), C.byref(ci), R, vp(o_px), vp(o_lm), vp(o_un), vp(o_bv), vp(o_desc),
                                                     vp(o_val), vp(o_col)))
            return (time.perf_counter() - t0) * 1e3
        L.check(lib.ov2_btracker_describe_brief(bt.h_trk, S, vp(px), vp(n), N, vp(d0), vp(v0)))
        t1 = time.perf_counter()
        L.check(lib.ov2_btracker_detect_singlescale(bt.h_trk, S, CELL, vp(px), vp(n), roi, vp(quality), 1, vp(det), cap, vp(det_n)))
        t2 = time.perf_counter()
        new_n[:] = np.minimum(det_n, N - n_prev)                          # (host work of a real route, kept out of the pieces below)
        m = int(new_n.max())
        new_pts[:, :m] = det[:, :m]; frame[:, n_prev:n_prev + m] = det[:, :m]
        t3 = time.perf_counter()
        L.check(lib.ov2_btracker_describe_brief(bt.h_trk, S, vp(new_pts), vp(new_n), N, vp(d1), vp(v1)))
        t4 = time.perf_counter()
        L.check(lib.ov2_compute_keypoints(ctx.h, cal.model, vp(cal.K), Dp, 0 if cal.D is None else len(cal.D), vp(cal.iK), vp(frame), S * N,
                                          vp(r_un), vp(r_bv)))
        t5 = time.perf_counter()
        for b in flagged:
            nk = n_prev + int(new_n[b])
            L.check(lib.ov2_btracker_set_keyframe(bt.h_trk, int(b), nk, vp(asc), vp(r_un[b]), vp(r_bv[b]), vp(Twc)))
            L.check(lib.ov2_btracker_set_keyframe_info(bt.h_trk, int(b), int(nkfid[b]), 12.5, 100))
        t6 = time.perf_counter()
        pieces.append(((t1 - t0) * 1e3, (t2 - t1) * 1e3, (t4 - t3) * 1e3, (t5 - t4) * 1e3, (t6 - t5) * 1e3))
        return sum(pieces[-1])

    forms = ["route", "fused"]
    res, rounds = {k: [] for k in forms}, {k: [] for k in forms}
    for r in range(ROUNDS):
        for form in forms:
            for _ in range(2):
                call(form)
            if form == "route":
                del pieces[-2:]
            ts = [call(form) for _ in range(K)]
            res[form] += ts
            rounds[form].append(float(np.median(ts)))
    q = lambda v: dict(median=float(np.median(v)), q1=float(np.percentile(v, 25)), q3=float(np.percentile(v, 75)))
    a = np.array(pieces)
    names = ("describe_brief_frame", "detect_singlescale", "describe_brief_new", "compute_keypoints", "set_keyframe_and_info")
    acts = [R[int(b)].action for b in flagged]
    line = json.dumps(dict(S=S, flag=FLAG, flagged=int(len(flagged)), calls=K, rounds=ROUNDS, ms={k: q(v) for k, v in res.items()},
                           round_medians_ms=rounds, route_pieces_ms={k: q(a[:, j]) for j, k in enumerate(names)},
                           last_fused_call=dict(created_share=float(np.mean([x == L.OV2_CKF_CREATED for x in acts])),
                                                n_new_mean=float(np.mean([R[int(b)].n_new for b in flagged])),
                                                n_kf_mean=float(np.mean([R[int(b)].n_kf for b in flagged])))))
    print(line)
    if OUT:
        with open(OUT, "a") as fh:
            fh.write(line + "\n")
    bt.close(); ctx.close()


if __name__ == "__main__":
    main()
