"""Wall and device time of the device epipolar2d2dFiltering chain (csrc/epifilter.hip) against the route of separate calls it
replaces, on the same GPU in the same process, alternating:

    python tools/epifilter_time.py [reps] [output.json, default profiles/epifilter_time.json]
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/epifilter_time.py --one 11 5       (per-kernel times of one case)

Workload: 308 keypoints against a 308-keypoint keyframe, 200 of them 3-D, 30 % mismatches among the matches the search sees,
100 iterations over 200 sample rows, the stereo form with the Sampson pass (8 distinct scenes repeated).  Cases: one frame, batches
of 11 and 4096.

    chain   ov2_epipolar_filter[_batch]: one upload, five launches, one download, one synchronisation.
    route   ov2_parallax_batch(AVG_WIDE) -> join on the host -> ov2_epipolar_draw_samples per item -> ov2_epipolar_ransac_batch ->
            F on the host -> ov2_sampson_filter_2d_batch: three synchronisations, two more staging passes.  Its time is reported in
            three parts: `calls` (the three C calls), `draw` (the C draw), `host` (the join, the ctypes packing and F in numpy -- a C++
            caller would spend less there, so the ratio is given both with and without it).

Prints one JSON line (and writes it): per case the median and the quartiles (us) of the wall time of both routes, the device time of
the chain (two events on the context's stream around the call: both copies and the five kernels), and the ratios route / chain.
Each case runs in a child process of its own under a time limit; a case whose child fails or times out is reported as null and ends
the run."""
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CASES = [0, 11, 4096]
ROWS = 200


def _q(v):
    v = np.asarray(v, np.float64) * 1e6
    return dict(median=float(np.median(v)), q1=float(np.percentile(v, 25)), q3=float(np.percentile(v, 75)), n=int(len(v)))


def _fundamental_batch(K, models):
    """inv(K).T hat(t) R inv(K) per model, vectorised (timing only: the bits are the specification's business)"""
    fx, fy, cx, cy = K
    iK = np.linalg.inv(np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]]))
    Rm, t = models[:, :9].reshape(-1, 3, 3), models[:, 9:]
    hat = np.zeros((len(models), 3, 3))
    hat[:, 0, 1], hat[:, 0, 2], hat[:, 1, 0], hat[:, 1, 2], hat[:, 2, 0], hat[:, 2, 1] = -t[:, 2], t[:, 1], t[:, 2], -t[:, 0], -t[:, 1], t[:, 0]
    return (iK.T @ hat @ Rm @ iK).reshape(-1, 9)


def measure(B, reps):
    import torch
    import ov2slam_amd
    from ov2slam_amd import keyframe, pose
    from ov2slam_amd import _lib as L
    from tests import epifilter_ref as R
    stream = torch.cuda.Stream()
    ctx = ov2slam_amd.Context(0, stream=stream.cuda_stream)
    P = R.make_P(stereo=True, n_rows=ROWS, max_iterations=100)
    base = [R.flatten(*R.geo_scene(900 + k, 308, n3d=200, outliers=60, outliers_2d=32, extra_kf=0)) for k in range(8)]
    nb = max(B, 1)
    items = [base[b % 8] for b in range(nb)]
    # ---- the chain: structs packed once, the call alone is timed
    p = keyframe._as_epifilter_params(dict(fkf=P["fkf"], max_iterations=P["max_iterations"], threshold=P["threshold"],
                                           fransac_err=P["fransac_err"], mono=False, n_rows=ROWS))
    S, Rr, keep = (L.EpifilterItem * nb)(), (L.EpifilterResult * nb)(), []
    for b in range(nb):
        S[b], k = keyframe._epifilter_item(items[b])
        Rr[b], o = keyframe._epifilter_result(S[b].fkf.n_cur, ROWS, False)
        keep.append((k, o))
    if B == 0:
        chain = lambda: L.check(ctx.lib.ov2_epipolar_filter(ctx.h, C.byref(p), S, Rr))
    else:
        chain = lambda: L.check(ctx.lib.ov2_epipolar_filter_batch(ctx.h, C.byref(p), B, S, Rr))
    # ---- the route
    fp = keyframe._as_fkf_params(P["fkf"])
    FS = (L.FkfItem * nb)()
    for b in range(nb):
        FS[b] = S[b].fkf
    PR = (L.ParallaxResult * nb)()
    ep = pose.epipolar_params(P["max_iterations"], P["threshold"], P["probability"])
    SR = (L.Sampson2dResult * nb)()
    souts = []
    for b in range(nb):
        SR[b], o = keyframe._sampson_result(FS[b].n_cur)
        souts.append(o)
    last = {}

    def route():
        t0 = time.perf_counter()
        L.check(ctx.lib.ov2_parallax_batch(ctx.h, C.byref(fp), nb, FS, 1, L.OV2_FKF_ONLY_3D, L.OV2_FKF_AVG_WIDE, PR))
        t1 = time.perf_counter()
        pbs = []
        for b in range(nb):                                                     # the join of :492-512 on the host
            it = items[b]
            j = np.searchsorted(it["kf_lmid"], it["cur_lmid"])
            jj = np.minimum(j, len(it["kf_lmid"]) - 1)
            pc = np.nonzero((it["kf_lmid"][jj] == it["cur_lmid"]) & (it["cur_is3d"] != 0))[0]
            pbs.append(dict(bv1=it["kf_bv"][jj[pc]], bv2=it["cur_bv"][pc], pair_cur=pc))
        t2 = time.perf_counter()
        for b in range(nb):
            pbs[b]["samples"] = pose.epipolar_draw_samples(items[b]["seed"], len(pbs[b]["pair_cur"]), ROWS)
        t3 = time.perf_counter()
        ES, ER, ekeep = (L.EpipolarProblem * nb)(), (L.EpipolarResult * nb)(), []
        for b in range(nb):
            ES[b], ER[b], k = pose._epi_problem(pbs[b], False)
            ekeep.append(k)
        t4 = time.perf_counter()
        L.check(ctx.lib.ov2_epipolar_ransac_batch(ctx.h, C.byref(ep), nb, ES, ER))
        t5 = time.perf_counter()
        models = np.array([ER[b].model[:] for b in range(nb)], np.float64)
        F = np.ascontiguousarray(_fundamental_batch(P["fkf"]["K"], models))
        t6 = time.perf_counter()
        L.check(ctx.lib.ov2_sampson_filter_2d_batch(ctx.h, nb, FS, F.ctypes.data_as(C.POINTER(C.c_double)), float(P["fransac_err"]), SR))
        t7 = time.perf_counter()
        last.update(n_out=int(ER[0].n_outliers), n_bad=int(SR[0].n_bad))
        return (t1 - t0) + (t5 - t4) + (t7 - t6), t3 - t2, (t2 - t1) + (t4 - t3) + (t6 - t5)

    chain(); route()                                                            # warm-up: code objects, scratch growth
    cw, cd, rc_, rd, rh = [], [], [], [], []
    for _ in range(reps):                                                       # alternating
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        t0 = time.perf_counter(); chain(); cw.append(time.perf_counter() - t0)
        e1.record(stream)
        e1.synchronize()
        cd.append(e0.elapsed_time(e1) * 1e-3)
        a, b, c = route()
        rc_.append(a); rd.append(b); rh.append(c)
    assert int(Rr[0].action) == R.FILTERED and int(Rr[0].n_removed_ransac) == last["n_out"] and int(Rr[0].n_removed_sampson) == last["n_bad"]
    name = "single" if B == 0 else "batch%d" % B
    rt = np.array(rc_) + np.array(rd) + np.array(rh)
    rcd = np.array(rc_) + np.array(rd)
    r = {name: dict(chain_wall_us=_q(cw), chain_device_us=_q(cd), route_calls_us=_q(rc_), route_draw_us=_q(rd), route_host_us=_q(rh),
                    route_total_us=_q(rt), route_calls_plus_draw_us=_q(rcd),
                    route_total_over_chain=float(np.median(rt) / np.median(cw)),
                    route_calls_plus_draw_over_chain=float(np.median(rcd) / np.median(cw)),
                    route_calls_over_chain=float(np.median(rc_) / np.median(cw)),
                    m=int(Rr[0].m), iterations=int(Rr[0].iterations), removed_ransac=int(Rr[0].n_removed_ransac),
                    removed_sampson=int(Rr[0].n_removed_sampson))}
    ctx.close()
    return r


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--one":
        print(json.dumps(measure(int(sys.argv[2]), int(sys.argv[3]))))
        return 0
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 30
    path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "epifilter_time.json")
    res, rc = {"n_cur": 308, "n_kf": 308, "n_3d": 200, "rows": ROWS, "max_iterations": 100}, 0
    for B in CASES:                                                           # one fresh process per case, each under its own limit
        n = reps if B <= 64 else max(3, reps // 6)
        try:
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", str(B), str(n)], capture_output=True, text=True,
                                 timeout=150 if B <= 64 else 420)
        except subprocess.TimeoutExpired:
            out = None
        if out is None or out.returncode != 0:
            res["single" if B == 0 else "batch%d" % B] = None
            sys.stderr.write("epifilter_time: case %d failed%s\n" % (B, "" if out is None else ": " + out.stderr[-2000:]))
            rc = 1
            break
        res.update(json.loads(out.stdout.strip().splitlines()[-1]))
    line = json.dumps(res)
    print(line)
    with open(path, "w") as f:
        f.write(line + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
