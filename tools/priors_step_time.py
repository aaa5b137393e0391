"""Step time of the lock-step tracker with the priors supplied by the host (ov2_btracker_track_frame) and derived on the device
inside the step (ov2_btracker_track_frame_map), S sequences of 752 x 480 with 308 keypoints each:

    python tools/priors_step_time.py [S] [steps] [rounds] [--tree DIR]

--tree DIR imports the package from another checkout (a build of the parent commit: only the host-prior form exists there and only
it is timed), so that both builds can be measured by the same tool in one session, alternating.  The frames sit in the tracker's
pinned staging sets, every argument is prepared outside the timed region, and a step ends in its host synchronisation: the time is
the C call.  Forms: `host` = track_frame with priors computed ahead (their cost is NOT in the step); `host+priors` = the same with
ov2_klt_priors_batch inside the timed step; `map` = track_frame_map.  Prints one JSON line with the median ms per step of every
round and the share of keypoints tracked over the timed steps of the last round (with steps a multiple of 3 the forms agree on it)."""
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
sys.path.insert(0, TREE)

import ov2slam_amd                                                 # noqa: E402
from ov2slam_amd import _lib as L                                  # noqa: E402
from ov2slam_amd.batch import SyntheticSequence                    # noqa: E402
from tests.match_ref import RADTAN4, EUROC, _inv_act, _rand_pose, in_image, make_params, project_dist   # noqa: E402
from tests.tri_ref import D, pose, se3_act                         # noqa: E402

S = int(argv[0]) if len(argv) > 0 else 4096
K = int(argv[1]) if len(argv) > 1 else 30
ROUNDS = int(argv[2]) if len(argv) > 2 else 3
W, H, N = 752, 480, 308
HAS_MAP = "ov2_btracker_track_frame_map" in L.SIGNATURES


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
    from ov2slam_amd import synth
    P = make_params(D=RADTAN4)
    # per step kind (the frame enters staging set f % 3 and shows view f % 3): keypoints, the map points whose projection under the
    # predicted pose is the true position (+ noise), and the priors a host would derive from them
    kinds = []
    for v in range(3):
        per_c = []
        for c in range(8):
            k = synth.grid_keypoints(W, H, 35, rng)[:N].astype(np.float32)
            k = np.concatenate([k, k[:N - len(k)]]) if len(k) < N else k
            gt = (seqs[c].flow(k.astype(np.float64), (v + 2) % 3, v) + rng.normal(0, 0.7, (N, 2))).astype(np.float32)
            T = _rand_pose(rng)
            unpx, bv = cal.computeKeypoints(gt)
            is3d = (rng.uniform(size=N) < 0.7).astype(np.uint8)
            wpt = np.stack([_inv_act(T, bv[i] / bv[i][2] * rng.uniform(2, 10)) for i in range(N)])
            pri, hp = k.copy(), np.zeros(N, np.uint8)
            for i in range(N):
                if is3d[i]:
                    pr = project_dist(P, se3_act(pose(T), tuple(D(x) for x in wpt[i])))
                    if in_image(P, pr):
                        pri[i], hp[i] = pr, 1
            per_c.append((k, wpt, is3d, T, pri, hp))
        idx = np.arange(S) % 8
        kinds.append(dict(kps=np.ascontiguousarray(np.stack([p[0] for p in per_c])[idx]), wpt=np.ascontiguousarray(np.stack([p[1] for p in per_c])[idx]),
                          is3d=np.ascontiguousarray(np.stack([p[2] for p in per_c])[idx]), Tcw=np.ascontiguousarray(np.stack([p[3] for p in per_c])[idx]),
                          pri=np.ascontiguousarray(np.stack([p[4] for p in per_c])[idx]), hp=np.ascontiguousarray(np.stack([p[5] for p in per_c])[idx])))
    n = np.full(S, N, np.int32)
    out = np.zeros((S, N, 2), np.float32); st = np.zeros((S, N), np.uint8); p3p = np.zeros(S, np.int32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    stride = bt.stride
    if HAS_MAP:
        from ov2slam_amd import priors as PR
        pk = PR._as_klt_params(dict(P, klt_use_prior=True))
        batch_args = []
        for kd in kinds:
            SK, RK = (L.KltPriorsItem * S)(), (L.KltPriorsResult * S)()
            pri2, hp2 = np.zeros((S, N, 2), np.float32), np.zeros((S, N), np.uint8)
            for b in range(S):
                SK[b].Tcw = kd["Tcw"][b].ctypes.data_as(C.POINTER(C.c_double)); SK[b].n = N
                SK[b].px = kd["kps"][b].ctypes.data_as(C.POINTER(C.c_float)); SK[b].is3d = kd["is3d"][b].ctypes.data_as(C.POINTER(C.c_uint8))
                SK[b].wpt = kd["wpt"][b].ctypes.data_as(C.POINTER(C.c_double))
                RK[b].prior = pri2[b].ctypes.data_as(C.POINTER(C.c_float)); RK[b].has_prior = hp2[b].ctypes.data_as(C.POINTER(C.c_uint8))
            batch_args.append((SK, RK, pri2, hp2))

    def step(form, f):
        which = f % 3
        kd = kinds[which]
        if form == "map":
            L.check(lib.ov2_btracker_track_frame_map(bt.h_trk, S, ptrs[which], stride, vp(kd["kps"]), vp(kd["wpt"]), vp(kd["is3d"]), vp(kd["Tcw"]),
                                                     vp(n), 1, vp(out), vp(st), vp(p3p)))
            return
        pri, hp = kd["pri"], kd["hp"]
        if form == "host+priors":
            SK, RK, pri, hp = batch_args[which]
            L.check(lib.ov2_klt_priors_batch(ctx.h, C.byref(pk), S, SK, RK))
        L.check(lib.ov2_btracker_track_frame(bt.h_trk, S, ptrs[which], stride, vp(kd["kps"]), vp(pri), vp(hp), vp(n), 1, vp(out), vp(st), vp(p3p)))

    forms = ["host", "host+priors", "map"] if HAS_MAP else ["host"]
    res = {k: [] for k in forms}
    tracked = {}
    f = 0
    for _ in range(3):
        step("host", f); f += 1
    for r in range(ROUNDS):
        for form in forms:
            for _ in range(3):
                step(form, f); f += 1
            t, ok = time.perf_counter(), []
            for _ in range(K):
                step(form, f); f += 1
                ok.append(int(np.count_nonzero(st[::64] & 1)))          # (a cheap sample: every 64th item)
            res[form].append((time.perf_counter() - t) / K * 1e3)
            tracked[form] = float(np.sum(ok)) / (K * st[::64].size)
    bt.close(); ctx.close()
    print(json.dumps(dict(tree=os.path.basename(TREE), S=S, steps=K, ms_per_step=res, median_ms={k: float(np.median(v)) for k, v in res.items()},
                          tracked=tracked, p3p_requests=int(p3p.sum()))))


if __name__ == "__main__":
    main()
