"""Time of Mapper::triangulateTemporal on the resident keyframe for the flagged items of a lock-step batch as one call
(ov2_btracker_temporal_keyframe) against the route of separate calls it replaces: S sequences of 752 x 480, 308 slots per item (one
keypoint in every cell of the 35 px grid), 70 % of them 3-D, a keyframe 0.3 m to the right of the one every keypoint anchors at:

    python tools/temporalkf_time.py [S] [calls] [rounds] [--flag all|fifth] [--out FILE]

The method of tools/stereokf_time.py: one process, the forms alternate call by call, every argument is prepared outside the timed
region, every call is timed on its own and ends in its own host synchronisation; the median and the quartiles of all timed calls are
reported.  In front of every timed call of any form, outside the timed region, the anchor tables of the flagged items are installed
again as they were before the keyframe (ov2_btracker_set_anchors) and the slots the last call made 3-D are made 2-D again (one
ov2_btracker_update_frame_batch of UNSET ops), so that every call does the same work: the table moves on to the new keyframe and
every 2-D slot is triangulated against the first keyframe.  --flag fifth: one item in five is flagged.  Forms:
  fused        ov2_btracker_temporal_keyframe
  route_calls  the route's C calls alone, on arguments that lie ready: ov2_triangulate_keyframe_batch,
               ov2_btracker_update_frame_batch and ov2_btracker_set_keyframe_info per flagged item (the scene has no REMOVE_OBS, so
               no ov2_btracker_set_keyframe).  A lower bound of any route.
  route_host   the route with its host anchor walk: ov2_btracker_get_frame (the mirror) per flagged item, the walk in numpy (the
               joins of the frame against the keyframe and the table by searchsorted, the new table, src / src_unpx / src_bv),
               composing the SET ops from the statuses, and the calls above.
Prints one JSON line (and appends it to --out)."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

argv = list(sys.argv[1:])
TREE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPT = {"--flag": "all", "--out": None}
for flag in list(OPT):
    if flag in argv:
        i = argv.index(flag)
        OPT[flag] = argv[i + 1]
        del argv[i:i + 2]
sys.path.insert(0, TREE)

import ov2slam_amd                                                 # noqa: E402
from ov2slam_amd import _lib as L                                  # noqa: E402
from ov2slam_amd import mapper                                     # noqa: E402
from ov2slam_amd.batch import SyntheticSequence                    # noqa: E402
from tests.match_ref import EUROC                                  # noqa: E402
from tests.stereokf_ref import se3_inverse                         # noqa: E402

S = int(argv[0]) if len(argv) > 0 else 4096
K = int(argv[1]) if len(argv) > 1 else 6
ROUNDS = int(argv[2]) if len(argv) > 2 else 1
FLAG, OUT = OPT["--flag"], OPT["--out"]
W, H, N, CELL, N_SRC = 752, 480, 308, 35, 8
NBW, NBH = (W + CELL - 1) // CELL, (H + CELL - 1) // CELL          # the frame grid: 22 x 14 = 308 cells
OPDT = np.dtype([("lmid", np.int32), ("op", np.int32), ("xyz", np.float64, 3)])      # ov2_resident_op


def main():
    ctx = ov2slam_amd.Context(0)
    lib = ctx.lib
    Kc = EUROC["K"]
    cal = ov2slam_amd.CameraCalibration(ctx, "pinhole", *Kc, D=None)
    bt = ov2slam_amd.LockstepTracker(ctx, S, W, H, use_clahe=False, nbmaxkps=N)
    bt.setCalibration(cal)
    bt.reserveAnchors(N_SRC)
    rng = np.random.default_rng(5)
    seqs = [SyntheticSequence("s%d" % c, 3, 100 + c, n_views=3) for c in range(8)]      # 8 image contents
    for b in range(S):
        bt.image_buffers[0][b][:, :W] = seqs[b % 8].views[0]
    z2 = np.zeros((S, N, 2), np.float32)
    bt.trackFrame([bt.image_buffers[0][b] for b in range(S)], z2, z2, None, np.zeros(S, np.int32))      # the current frame: pyramid and raw
    ctx.sync()
    # one keypoint per cell of the frame grid at keyframe 1, the point behind it 3 .. 7 m away, its pixel at keyframe 0 (0.3 m to the
    # left); 70 % of the slots 3-D
    T0, T1 = np.array([0.0, -0.2, 0.1, 0.0, 0.0, 0.0, 1.0]), np.array([0.3, -0.2, 0.1, 0.0, 0.0, 0.0, 1.0])
    Km = np.array([[Kc[0], 0, Kc[2]], [0, Kc[1], Kc[3]], [0, 0, 1.0]])
    iK = np.linalg.inv(Km)
    frames = []
    for c8 in range(8):
        p1 = np.array([(min(CELL * c + rng.uniform(6, 29), W - 12), min(CELL * r + rng.uniform(6, 29), H - 12))
                       for r in range(NBH) for c in range(NBW)], np.float32)[rng.permutation(N)]
        Pc = (iK @ np.concatenate([p1.astype(np.float64), np.ones((N, 1))], 1).T).T * rng.uniform(3, 7, (N, 1))
        X = Pc + T1[:3]
        q = (Km @ (X - T0[:3]).T).T
        p0 = (q[:, :2] / q[:, 2:]).astype(np.float32)
        d3 = (rng.uniform(size=N) < 0.7).astype(np.uint8)
        frames.append((p0, p1, rng.permutation(1000)[:N].astype(np.int32), d3, X))
    state = np.full(S, 1e-3)
    ckp = dict(ncellsize=CELL, nbwcells=NBW, nbhcells=NBH, nbmaxkps=0, detector="singlescale", det_cell=CELL, roi=(5, 5, W - 10, H - 10),
               mask_mode=0, do_subpix=True, use_brief=False)
    tri = mapper.tri_params(Kc, iK, Kc, (0.11, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0), (-0.11, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0), stereo=False, rect=False,
                            fmax_reproj_err=3.0)
    tkp = mapper.temporal_keyframe_params(tri, n_src_max=N_SRC)
    do_all = np.ones(S, np.uint8)
    vp = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
    R = (L.TemporalKeyframeResult * S)()
    o_st, o_w, o_inv, o_kf = np.zeros((S, N), np.uint8), np.zeros((S, N, 3)), np.zeros((S, N)), np.zeros((S, N), np.int32)
    kfs = []
    for k, T in enumerate((T0, T1)):                                          # keyframe 0 (pixels out of the image are fine: nothing reads them)
        for b in range(S):
            p0, p1, lm, d3, X = frames[b % 8]
            bt.setPose(b, T)
            bt.setFrame(b, np.clip(p0, 0, [W - 1, H - 1]) if k == 0 else p1, lm, d3, X)
        recs, o = bt.createKeyframe(S, None, None, None, None, do_all, np.full(S, 1000, np.int32), np.full(S, k + 1, np.int32),
                                    np.full(S, 12.5 + k), ckp, state)
        assert all(r["action"] == L.OV2_CKF_CREATED and r["n_kf"] == N for r in recs)
        kfs.append(o)
        if k == 0:
            L.check(lib.ov2_btracker_temporal_keyframe(bt.h_trk, S, C.byref(tkp), vp(do_all), R, vp(o_st), vp(o_w), vp(o_inv), vp(o_kf)))
    do = do_all if FLAG == "all" else (np.arange(S) % 5 == 0).astype(np.uint8)
    flagged = [int(b) for b in np.nonzero(do)[0]]
    F = len(flagged)
    # the tables before keyframe 1, as the tracker holds them (one per image content), and keyframe 1's arrays sorted by lmid
    tab0 = [bt.getAnchors(c8, False) for c8 in range(min(8, S))]
    kf1 = []
    for c8 in range(min(8, S)):
        order = np.argsort(kfs[1]["lmid"][c8, :N], kind="stable")
        kf1.append(dict(lmid=kfs[1]["lmid"][c8, :N][order].copy(), unpx=kfs[1]["unpx"][c8, :N][order].copy(), bv=kfs[1]["bv"][c8, :N][order].copy()))
    Tcw0 = se3_inverse(lib, T0)
    # ---- the route's buffers: slot layout over the whole batch
    px, lm_all, d3_all, wpt = np.zeros((S, N, 2), np.float32), np.zeros((S, N), np.int32), np.zeros((S, N), np.uint8), np.zeros((S, N, 3))
    unpx, bv, sun, sbv, src = np.zeros((S, N, 2), np.float32), np.zeros((S, N, 3)), np.zeros((S, N, 2), np.float32), np.zeros((S, N, 3)), np.zeros((S, N), np.int32)
    srcT, srcTi = np.zeros((S, N_SRC, 7)), np.zeros((S, N_SRC, 7))
    tst, tw, tinv = np.zeros((S, N), np.uint8), np.zeros((S, N, 3)), np.zeros((S, N))
    TK, TR = (L.TriKeyframe * F)(), (L.TriResult * F)()
    fp, dp, ip, up = C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_uint8)
    at = lambda a, b, t: C.cast(a[b].ctypes.data, t)
    T1c = np.ascontiguousarray(T1)
    for j, b in enumerate(flagged):
        TK[j].n, TK[j].Twc, TK[j].unpx, TK[j].bv = N, T1c.ctypes.data_as(dp), at(unpx, b, fp), at(bv, b, dp)
        TK[j].src, TK[j].src_unpx, TK[j].src_bv = at(src, b, ip), at(sun, b, fp), at(sbv, b, dp)
        TK[j].n_src, TK[j].src_Twc, TK[j].src_Tcw = 2, at(srcT, b, dp), at(srcTi, b, dp)
        TR[j].status, TR[j].wpt, TR[j].invdepth = at(tst, b, up), at(tw, b, dp), at(tinv, b, dp)
    OPS = {code: (np.zeros(S * N, OPDT), (C.POINTER(L.ResidentOp) * S)(), np.zeros(S, np.int32)) for code in (L.OV2_RES_SET_POINT, L.OV2_RES_UNSET_POINT)}
    UR = (L.ResidentUpdateResult * S)()
    pieces = []

    def pack_ops(code, status):
        """one op per OV2_TRI_TEMPORAL_OK slot of the flagged items: SET with the point (the route's) or UNSET (putting the frames back)"""
        ops, op_ptr, n_ops = OPS[code]
        at_ = 0
        n_ops[:] = 0
        for b in flagged:
            sel = np.nonzero(status[b] & L.OV2_TRI_TEMPORAL_OK)[0]
            m = len(sel)
            o = ops[at_:at_ + m]
            o["lmid"], o["op"] = lm_all[b, sel], code
            o["xyz"] = tw[b, sel] if code == L.OV2_RES_SET_POINT else 0.0
            n_ops[b] = m
            op_ptr[b] = C.cast(ops.ctypes.data + OPDT.itemsize * at_, C.POINTER(L.ResidentOp))
            at_ += m

    def host_walk():
        """what a caller of the route does on the host: the frames out of the mirror, the anchor walk, the triangulation's inputs"""
        n = C.c_int()
        for b in flagged:
            L.check(lib.ov2_btracker_get_frame(bt.h_trk, b, 0, C.byref(n), vp(px[b]), vp(lm_all[b]), vp(d3_all[b]), vp(wpt[b])))
            kf, tb = kf1[b % 8], tab0[b % 8]
            # the new table: a keypoint the old table holds inherits, another anchors here; the rows still referred to, then this one
            e = np.searchsorted(tb["lmid"], kf["lmid"])
            e[e >= tb["n"]] = 0
            hit = tb["lmid"][e] == kf["lmid"] if tb["n"] else np.zeros(N, bool)
            a_kf = np.where(hit, tb["kfid"][e], 2)
            a_un = np.where(hit[:, None], tb["unpx"][e], kf["unpx"])
            a_bv = np.where(hit[:, None], tb["bv"][e], kf["bv"])
            rows = np.unique(a_kf[hit])
            rows = np.concatenate([rows, [2]])
            assert len(rows) <= N_SRC
            srcT[b, 0], srcTi[b, 0], srcT[b, 1], srcTi[b, 1] = tb["row_Twc"][0], Tcw0, T1, 0.0
            # the frame's slots joined against the keyframe (sorted by lmid: the table's order too)
            j = np.searchsorted(kf["lmid"], lm_all[b])
            j[j >= N] = 0
            inkf = kf["lmid"][j] == lm_all[b]
            unpx[b], bv[b] = np.where(inkf[:, None], kf["unpx"][j], 0), np.where(inkf[:, None], kf["bv"][j], 0)
            sun[b], sbv[b] = np.where(inkf[:, None], a_un[j], 0), np.where(inkf[:, None], a_bv[j], 0)
            src[b] = np.where(inkf & (a_kf[j] != 2) & (d3_all[b] == 0), np.searchsorted(rows, a_kf[j]), -1)

    def route_calls(compose):
        t0 = time.perf_counter()
        L.check(lib.ov2_triangulate_keyframe_batch(ctx.h, C.byref(tri), F, TK, TR))
        t1 = time.perf_counter()
        if compose:
            pack_ops(L.OV2_RES_SET_POINT, tst)
        t2 = time.perf_counter()
        L.check(lib.ov2_btracker_update_frame_batch(bt.h_trk, S, OPS[L.OV2_RES_SET_POINT][2].ctypes.data_as(ip), OPS[L.OV2_RES_SET_POINT][1], UR))
        t3 = time.perf_counter()
        for b in flagged:
            L.check(lib.ov2_btracker_set_keyframe_info(bt.h_trk, b, 2, 13.5, 200))
        t4 = time.perf_counter()
        pieces.append(((t1 - t0) * 1e3, (t3 - t2) * 1e3, (t4 - t3) * 1e3))
        return sum(pieces[-1]), (t2 - t1) * 1e3

    def put_back(status):
        """outside every timed region: the new 3-D slots 2-D again, the flagged items' tables as they were before the keyframe"""
        pack_ops(L.OV2_RES_UNSET_POINT, status)
        L.check(lib.ov2_btracker_update_frame_batch(bt.h_trk, S, OPS[L.OV2_RES_UNSET_POINT][2].ctypes.data_as(ip), OPS[L.OV2_RES_UNSET_POINT][1], UR))
        for b in flagged:
            tb = tab0[b % 8]
            bt.setAnchors(b, tb["lmid"], tb["kfid"], tb["unpx"], tb["bv"], tb["row_kfid"], tb["row_Twc"])

    def call(form):
        if form == "fused":
            t0 = time.perf_counter()
            L.check(lib.ov2_btracker_temporal_keyframe(bt.h_trk, S, C.byref(tkp), vp(do), R, vp(o_st), vp(o_w), vp(o_inv), vp(o_kf)))
            ms = (time.perf_counter() - t0) * 1e3
            tw[:] = o_w
            put_back(o_st)
            return ms
        if form == "route_calls":
            ms, _ = route_calls(False)                                        # the inputs and the ops: those of the warm-up call
        else:
            t0 = time.perf_counter()
            host_walk()
            host = (time.perf_counter() - t0) * 1e3
            calls, compose = route_calls(True)
            ms = host + calls + compose
        put_back(tst)
        return ms

    # the route's arguments once, outside every timed region (route_calls works on these; route_host rebuilds them inside its timing)
    host_walk()
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
    names = ("triangulate_keyframe_batch", "update_frame_batch", "set_keyframe_info")
    same = bool(np.array_equal(o_st[flagged], tst[flagged]) and np.array_equal(o_w[flagged].view(np.uint64), tw[flagged].view(np.uint64)))
    line = json.dumps(dict(S=S, flag=FLAG, flagged=F, calls=K, rounds=ROUNDS, ms={k: q(v) for k, v in res.items()},
                           route_pieces_ms={k: q(a[:, j]) for j, k in enumerate(names)},
                           last_fused_call=dict(done_share=float(np.mean([R[b].action == L.OV2_TKF_DONE for b in flagged])),
                                                n_candidates_mean=float(np.mean([R[b].n_candidates for b in flagged])),
                                                n_temporal_good_mean=float(np.mean([R[b].n_temporal_good for b in flagged])),
                                                n_rows_mean=float(np.mean([R[b].n_rows for b in flagged])),
                                                statuses_and_points_equal_the_routes=same)))
    print(line)
    if OUT:
        with open(OUT, "a") as fh:
            fh.write(line + "\n")
    bt.close(); ctx.close()


if __name__ == "__main__":
    main()
