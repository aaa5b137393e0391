"""Time of the mapper's stereo block on the resident keyframe (MapManager::stereoMatching, then Mapper::triangulateStereo) for the
flagged items of a lock-step batch as one call (ov2_btracker_stereo_keyframe) against the route of separate calls it replaces:
S sequences of 752 x 480 with CLAHE, 308 slots per item (one keypoint in every cell of the 35 px grid), 70 % of them 3-D, a right
image at a constant disparity of 12 px:

    python tools/stereokf_time.py [S] [calls] [rounds] [--flag all|fifth] [--rect 0|1] [--out FILE]

The method of tools/createkf_time.py: one process, the forms alternate call by call, every argument is prepared outside the timed
region, every call is timed on its own and ends in its own host synchronisation; the median and the quartiles of all timed calls are
reported.  The right pyramid is built once, outside every timed region.  After every timed call of any form the slots that the call
made 3-D are made 2-D again (one untimed ov2_btracker_update_frame_batch of UNSET ops), so that every call does the same work.
--flag fifth: one item in five is flagged.  Forms:
  fused        ov2_btracker_stereo_keyframe
  route_calls  the route's C calls alone, on arguments prepared beforehand: ov2_stereo_priors_batch, ov2_stereo_match_batch,
               ov2_compute_keypoints of the right camera over every slot, ov2_triangulate_keyframe_batch,
               ov2_btracker_update_frame_batch and ov2_btracker_set_keyframe_info per flagged item.  A lower bound of any route.
  route_host   the route with its host work: ov2_btracker_get_frame (the mirror) per flagged item, ov2_compute_keypoints of the left
               camera, the numpy cell tables (tests/stereokf_ref.py: cell_tables), composing state / is_stereo / the SET ops from
               the statuses, and the calls above.
Prints one JSON line (and appends it to --out)."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

argv = list(sys.argv[1:])
TREE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPT = {"--flag": "all", "--rect": "1", "--out": None}
for flag in list(OPT):
    if flag in argv:
        i = argv.index(flag)
        OPT[flag] = argv[i + 1]
        del argv[i:i + 2]
sys.path.insert(0, TREE)

import ov2slam_amd                                                 # noqa: E402
from ov2slam_amd import _lib as L                                  # noqa: E402
from ov2slam_amd import mapper, priors                             # noqa: E402
from ov2slam_amd.batch import SyntheticSequence                    # noqa: E402
from tests.match_ref import EUROC                                  # noqa: E402
from tests.stereo_cases import F_XTRANS, RADTAN                    # noqa: E402
from tests.stereokf_ref import cell_tables, se3_inverse            # noqa: E402

S = int(argv[0]) if len(argv) > 0 else 4096
K = int(argv[1]) if len(argv) > 1 else 6
ROUNDS = int(argv[2]) if len(argv) > 2 else 1
FLAG, RECT, OUT = OPT["--flag"], int(OPT["--rect"]) != 0, OPT["--out"]
W, H, N, CELL, DISP, BASELINE = 752, 480, 308, 35, 12, 0.11
NBW, NBH = (W + CELL - 1) // CELL, (H + CELL - 1) // CELL          # the frame grid: 22 x 14 = 308 cells
OPDT = np.dtype([("lmid", np.int32), ("op", np.int32), ("xyz", np.float64, 3)])      # ov2_resident_op


def main():
    ctx = ov2slam_amd.Context(0)
    lib = ctx.lib
    Kc = EUROC["K"]
    Dc = None if RECT else RADTAN
    cal = ov2slam_amd.CameraCalibration(ctx, "pinhole", *Kc, D=Dc)          # identical cameras
    bt = ov2slam_amd.LockstepTracker(ctx, S, W, H, nbmaxkps=N)
    bt.setCalibration(cal)
    rng = np.random.default_rng(5)
    seqs = [SyntheticSequence("s%d" % c, 3, 100 + c, n_views=3, stereo=True, disparity=float(DISP)) for c in range(8)]      # 8 image contents
    for b in range(S):
        bt.image_buffers[0][b][:, :W] = seqs[b % 8].views[0]
    z2 = np.zeros((S, N, 2), np.float32)
    bt.trackFrame([bt.image_buffers[0][b] for b in range(S)], z2, z2, None, np.zeros(S, np.int32))      # the current frame: pyramid and raw
    rp = ov2slam_amd.Pyramid(ctx, W, H, 9, 3, batch=S)
    rp.build_clahe_batch([seqs[b % 8].right_views[0] for b in range(S)], 3.0, W // 50, H // 50)
    ctx.sync()
    # one keypoint per cell of the frame grid, 70 % of them 3-D with the point of the scene's plane behind the pixel
    Twc = np.array([0.3, -0.2, 0.1, 0.0, 0.0, 0.0, 1.0])
    iK = np.linalg.inv(np.array([[Kc[0], 0, Kc[2]], [0, Kc[1], Kc[3]], [0, 0, 1.0]]))
    z0 = Kc[0] * BASELINE / DISP
    frames = []
    for c8 in range(8):
        p = np.array([(min(CELL * c + rng.uniform(6, 29), W - 12), min(CELL * r + rng.uniform(6, 29), H - 12))
                      for r in range(NBH) for c in range(NBW)], np.float32)[rng.permutation(N)]
        d3 = (rng.uniform(size=N) < 0.7).astype(np.uint8)
        wpt = (iK @ np.concatenate([p.astype(np.float64), np.ones((N, 1))], 1).T).T * z0 + Twc[:3]
        frames.append((p, rng.permutation(1000)[:N].astype(np.int32), d3, wpt))
    for b in range(S):
        bt.setPose(b, Twc)
        bt.setFrame(b, *frames[b % 8])
    state = np.full(S, 1e-3)
    ckp = dict(ncellsize=CELL, nbwcells=NBW, nbhcells=NBH, nbmaxkps=0, detector="singlescale", det_cell=CELL, roi=(5, 5, W - 10, H - 10),
               mask_mode=0, do_subpix=True, use_brief=False)
    recs, _ = bt.createKeyframe(S, None, None, None, None, np.ones(S, np.uint8), np.full(S, 1000, np.int32), np.arange(S, dtype=np.int32),
                                np.full(S, 12.5), ckp, state)
    assert all(r["action"] == L.OV2_CKF_CREATED and r["n_kf"] == N for r in recs)
    do = np.ones(S, np.uint8) if FLAG == "all" else (np.arange(S) % 5 == 0).astype(np.uint8)
    flagged = [int(b) for b in np.nonzero(do)[0]]
    Tcic0 = (-BASELINE, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0)
    tri = mapper.tri_params(Kc, iK, Kc, (BASELINE, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0), Tcic0, stereo=True, rect=RECT, fmax_reproj_err=3.0)
    Frl = None if RECT else np.ascontiguousarray(F_XTRANS, np.float64).reshape(9)
    skp = mapper.stereo_keyframe_params(cal, tri, img_w=W, img_h=H, Tcic0=Tcic0, rect=RECT, Frl=Frl, ncellsize=CELL)
    pp = priors._as_stereo_params(dict(model="pinhole", K=Kc, D=Dc, img_w=float(W), img_h=float(H), ncellsize=CELL, rect=RECT, Tcic0=Tcic0))
    vp = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
    Tcw = se3_inverse(lib, Twc)
    # ---- outputs
    R = (L.StereoKeyframeResult * S)()
    o_rpx, o_ok, o_st = np.zeros((S, N, 2), np.float32), np.zeros((S, N), np.uint8), np.zeros((S, N), np.uint8)
    o_w, o_inv = np.zeros((S, N, 3)), np.zeros((S, N))
    # ---- the route's buffers: slot layout over the whole batch
    kps, unpx, bv = np.zeros((S, N, 2), np.float32), np.zeros((S, N, 2), np.float32), np.zeros((S, N, 3))
    wpt, st8 = np.zeros((S, N, 3)), np.zeros((S, N), np.uint8)
    pri, hp, skip = np.zeros((S, N, 2), np.float32), np.zeros((S, N), np.uint8), np.zeros((S, N), np.uint8)
    nn = np.zeros(S, np.int32)
    right, ok = np.zeros((S, N, 2), np.float32), np.zeros((S, N), np.uint8)
    runpx, rbv, isst = np.zeros((S, N, 2), np.float32), np.zeros((S, N, 3)), np.zeros((S, N), np.uint8)
    tst, tw, tinv = np.zeros((S, N), np.uint8), np.zeros((S, N, 3)), np.zeros((S, N))
    cs_all, ck_all = np.zeros((S, NBW * NBH + 1), np.int32), np.zeros((S, N), np.int32)
    F = len(flagged)
    PI, PR = (L.StereoPriorsItem * F)(), (L.StereoPriorsResult * F)()
    TK, TR = (L.TriKeyframe * F)(), (L.TriResult * F)()
    fp, dp, ip, up = C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_uint8)
    at = lambda a, b, t: C.cast(a[b].ctypes.data, t)
    Twc_c, Tcw_c = np.ascontiguousarray(Twc), np.ascontiguousarray(Tcw)
    for j, b in enumerate(flagged):
        PI[j].Tcw, PI[j].n = Tcw_c.ctypes.data_as(dp), N
        PI[j].px, PI[j].unpx, PI[j].bv, PI[j].wpt, PI[j].state = at(kps, b, fp), at(unpx, b, fp), at(bv, b, dp), at(wpt, b, dp), at(st8, b, up)
        PI[j].cell_start, PI[j].cell_kp = (None, None) if RECT else (at(cs_all, b, ip), at(ck_all, b, ip))
        PR[j].prior, PR[j].has_prior, PR[j].skip = at(pri, b, fp), at(hp, b, up), at(skip, b, up)
        TK[j].n, TK[j].Twc, TK[j].unpx, TK[j].bv = N, Twc_c.ctypes.data_as(dp), at(unpx, b, fp), at(bv, b, dp)
        TK[j].is_stereo, TK[j].runpx, TK[j].rbv = at(isst, b, up), at(runpx, b, fp), at(rbv, b, dp)
        TR[j].status, TR[j].wpt, TR[j].invdepth = at(tst, b, up), at(tw, b, dp), at(tinv, b, dp)
    # two op lists: the route's SET ops, and the UNSET ops that put the frames back after a timed call
    OPS = {code: (np.zeros(S * N, OPDT), (C.POINTER(L.ResidentOp) * S)(), np.zeros(S, np.int32)) for code in (L.OV2_RES_SET_POINT, L.OV2_RES_UNSET_POINT)}
    UR = (L.ResidentUpdateResult * S)()
    Dp, nD = (vp(cal.D), len(cal.D)) if cal.D is not None else (None, 0)
    lm_all = np.zeros((S, N), np.int32)
    pieces = []

    def pack_ops(code, status):
        """one op per OV2_TRI_STEREO_OK slot of the flagged items: SET with the point (the route's) or UNSET (putting the frames back)"""
        ops, op_ptr, n_ops = OPS[code]
        at_ = 0
        n_ops[:] = 0
        for b in flagged:
            sel = np.nonzero(status[b] & L.OV2_TRI_STEREO_OK)[0]
            m = len(sel)
            o = ops[at_:at_ + m]
            o["lmid"], o["op"] = lm_all[b, sel], code
            o["xyz"] = tw[b, sel] if code == L.OV2_RES_SET_POINT else 0.0
            n_ops[b] = m
            op_ptr[b] = C.cast(ops.ctypes.data + OPDT.itemsize * at_, C.POINTER(L.ResidentOp))
            at_ += m

    def host_inputs():
        """what a caller of the route builds on the host: the frames out of the mirror, unpx / bv, state, the cell tables"""
        n = C.c_int()
        for b in flagged:
            L.check(lib.ov2_btracker_get_frame(bt.h_trk, b, 0, C.byref(n), vp(kps[b]), vp(lm_all[b]), vp(st8[b]), vp(wpt[b])))
            nn[b] = n.value
        L.check(lib.ov2_compute_keypoints(ctx.h, cal.model, vp(cal.K), Dp, nD, vp(cal.iK), vp(kps), S * N, vp(unpx), vp(bv)))
        if not RECT:
            for b in flagged:
                cs_all[b], ck_all[b] = cell_tables(kps[b], W, H, CELL)

    def route_calls(compose):
        t0 = time.perf_counter()
        L.check(lib.ov2_stereo_priors_batch(ctx.h, C.byref(pp), F, PI, PR))
        t1 = time.perf_counter()
        L.check(lib.ov2_stereo_match_batch(ctx.h, lib.ov2_btracker_cur_pyr(bt.h_trk), rp.h_pyr, S, 9, 3, 30, 0.01, 30.0, 0.5, int(RECT), vp(Frl),
                                           cal.model, vp(cal.K), Dp, nD, N, vp(kps), vp(unpx), vp(pri), vp(hp), vp(nn), vp(right), vp(ok)))
        t2 = time.perf_counter()
        L.check(lib.ov2_compute_keypoints(ctx.h, cal.model, vp(cal.K), Dp, nD, vp(cal.iK), vp(right), S * N, vp(runpx), vp(rbv)))
        t3 = time.perf_counter()
        if compose:
            np.logical_and(ok != 0, st8 == 0, out=isst.view(bool))
        t4 = time.perf_counter()
        L.check(lib.ov2_triangulate_keyframe_batch(ctx.h, C.byref(tri), F, TK, TR))
        t5 = time.perf_counter()
        if compose:
            pack_ops(L.OV2_RES_SET_POINT, tst)
        t6 = time.perf_counter()
        L.check(lib.ov2_btracker_update_frame_batch(bt.h_trk, S, OPS[L.OV2_RES_SET_POINT][2].ctypes.data_as(ip), OPS[L.OV2_RES_SET_POINT][1], UR))
        t7 = time.perf_counter()
        for b in flagged:
            L.check(lib.ov2_btracker_set_keyframe_info(bt.h_trk, b, b, 12.5, 200))
        t8 = time.perf_counter()
        pieces.append(((t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3, (t5 - t4) * 1e3, (t7 - t6) * 1e3, (t8 - t7) * 1e3))
        return sum(pieces[-1]), (t4 - t3 + t6 - t5) * 1e3

    def put_back(status):
        pack_ops(L.OV2_RES_UNSET_POINT, status)
        L.check(lib.ov2_btracker_update_frame_batch(bt.h_trk, S, OPS[L.OV2_RES_UNSET_POINT][2].ctypes.data_as(ip), OPS[L.OV2_RES_UNSET_POINT][1], UR))

    def call(form):
        if form == "fused":
            t0 = time.perf_counter()
            L.check(lib.ov2_btracker_stereo_keyframe(bt.h_trk, S, C.byref(skp), rp.h_pyr, vp(do), R, vp(o_rpx), vp(o_ok), vp(o_st), vp(o_w), vp(o_inv)))
            ms = (time.perf_counter() - t0) * 1e3
            tw[:] = o_w
            put_back(o_st)
            return ms
        if form == "route_calls":
            ms, _ = route_calls(False)                                        # is_stereo and the ops: those of the warm-up call
        else:
            t0 = time.perf_counter()
            host_inputs()
            host = (time.perf_counter() - t0) * 1e3
            calls, compose = route_calls(True)
            ms = host + calls + compose
        put_back(tst)
        return ms

    # the route's arguments once, outside every timed region (route_calls works on these; route_host rebuilds them inside its timing)
    nn[:] = 0
    host_inputs()
    route_calls(True)
    put_back(tst)
    pieces.clear()
    forms = ["fused", "route_calls", "route_host"]
    res = {k: [] for k in forms}
    for form in forms:
        call(form); call(form)                                                # warm-up
    n_pieces0 = len(pieces)
    for r in range(ROUNDS):
        for _ in range(K):
            for form in forms:                                                # the forms alternate call by call
                res[form].append(call(form))
    q = lambda v: dict(median=float(np.median(v)), q1=float(np.percentile(v, 25)), q3=float(np.percentile(v, 75)))
    a = np.array(pieces[n_pieces0:])
    names = ("stereo_priors_batch", "stereo_match_batch", "compute_keypoints_right", "triangulate_keyframe_batch", "update_frame_batch",
             "set_keyframe_info")
    same = bool(np.array_equal(o_st[flagged], tst[flagged]) and np.array_equal(o_ok[flagged], ok[flagged]))
    line = json.dumps(dict(S=S, rect=int(RECT), flag=FLAG, flagged=F, calls=K, rounds=ROUNDS, ms={k: q(v) for k, v in res.items()},
                           route_pieces_ms={k: q(a[:, j]) for j, k in enumerate(names)},
                           last_fused_call=dict(done_share=float(np.mean([R[b].action == L.OV2_SKF_DONE for b in flagged])),
                                                n_stereo_kps_mean=float(np.mean([R[b].n_stereo_kps for b in flagged])),
                                                n_stereo_good_mean=float(np.mean([R[b].n_stereo_good for b in flagged])),
                                                statuses_equal_the_routes=same)))
    print(line)
    if OUT:
        with open(OUT, "a") as fh:
            fh.write(line + "\n")
    bt.close(); rp.close(); ctx.close()


if __name__ == "__main__":
    main()
