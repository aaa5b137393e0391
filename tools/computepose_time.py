"""Wall and device time of the per-frame pose on the GPU (csrc/pnp.hip), next to the route the parent commit offers for the same work:

    python tools/computepose_time.py [reps] [output.json, default profiles/computepose_time.json]
    python tools/computepose_time.py --one <case> <reps>                                   (one case, in this process)

Prints one JSON line (and writes it): medians after a warm-up call, in us, on 308-point frames (0.5 px noise, 10 % outliers;
8 distinct scenes repeated through a batch), the front end's settings (LMedS, 100 iterations over 200 rows; nmaxiter 5):
    pnp_single         ov2_ceres_pnp, one frame                       pose_single         ov2_compute_pose with P3P, one frame
    pnp_two_call       MultiViewGeometry.ceresPnP: the two blocking ov2_ba_solve calls with the host-side outlier test between
    parent_single      the parent's route for one frame: ov2_p3p_ransac, host compaction, then the two-call ceresPnP
    parent_11          that route 11 times in a row                   pose_11x1           ov2_compute_pose 11 times in a row
    pnp_batch11 / pnp_batch4096, pose_batch11 / pose_batch4096        the batched forms
wall = the call(s) as the caller sees them (packing, copies, launches, the synchronisation, unpacking); device = the time between
two events on the context's stream around them.  Each case runs in a child process of its own under a time limit; a case whose
child fails or times out is reported as null and ends the run.  The library is the one OV2SLAM_HIP_LIB names, if set (a build
with another PNP_THREADS: tools/build_variant.sh), and its path is recorded."""
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CASES = ["pnp_single", "pnp_two_call", "pose_single", "parent_single", "parent_11", "pose_11x1", "pnp_batch11", "pose_batch11",
         "pnp_batch4096", "pose_batch4096"]
N, ROWS, ITERS = 308, 200, 100


def measure(case, reps):
    import torch
    import ov2slam_amd
    from ov2slam_amd import pose
    from ov2slam_amd import _lib as L
    from tests import computepose_ref as R
    from tests import p3p_ref
    stream = torch.cuda.Stream()
    ctx = ov2slam_amd.Context(0, stream=stream.cuda_stream)
    params = R.params_of()
    params["p3p"]["max_iterations"] = ITERS
    base = []
    for k in range(8):
        pb = R.make_scene(500 + k, N, outlier_frac=0.1, do_p3p=True)
        pb["samples"] = pose.draw_samples(k, N, ROWS)
        base.append(pb)
    mvg = ov2slam_amd.MultiViewGeometry(ctx)
    Kl = [float(v) for v in R.K]

    def parent(pb):
        s = pose.p3p_ransac(ctx, params["p3p"], dict(bv=pb["bv"], X=pb["wpt"], samples=pb["samples"]))
        keep = np.ones(N, bool)
        keep[s["outliers"]] = False
        return mvg.ceresPnP(pb["unpx"][keep], pb["wpt"][keep], pb["scale"][keep], pose.pose_from_model(s["model"]), 5, R.CHI2TH, True, True, *Kl)

    B = int(case.split("batch")[1]) if "batch" in case else 0
    if B:
        pnp = case.startswith("pnp")
        S, Rr = ((L.PnPProblem if pnp else L.PoseProblem) * B)(), ((L.PnPResult if pnp else L.PoseResult) * B)()
        keep = []
        for b in range(B):
            S[b], Rr[b], k = (pose._pnp_problem if pnp else pose._pose_problem)(base[b % 8])
            keep.append(k)
        P = pose._as_pnp_params(params["pnp"]) if pnp else pose._as_pose_params(params)
        fn = ctx.lib.ov2_ceres_pnp_batch if pnp else ctx.lib.ov2_compute_pose_batch
        call = lambda: L.check(fn(ctx.h, C.byref(P), B, S, Rr))
    elif case in ("pnp_single", "pose_single"):
        pnp = case == "pnp_single"
        S, Rr, keep = (pose._pnp_problem if pnp else pose._pose_problem)(base[0])
        P = pose._as_pnp_params(params["pnp"]) if pnp else pose._as_pose_params(params)
        fn = ctx.lib.ov2_ceres_pnp if pnp else ctx.lib.ov2_compute_pose
        call = lambda: L.check(fn(ctx.h, C.byref(P), C.byref(S), C.byref(Rr)))
    elif case == "pnp_two_call":
        pb = base[0]
        call = lambda: mvg.ceresPnP(pb["unpx"], pb["wpt"], pb["scale"], pb["Twc"], 5, R.CHI2TH, True, True, *Kl)
    elif case == "parent_single":
        call = lambda: parent(base[0])
    elif case == "parent_11":
        call = lambda: [parent(base[b % 8]) for b in range(11)]
    elif case == "pose_11x1":
        call = lambda: [pose.compute_pose(ctx, params, base[b % 8]) for b in range(11)]
    else:
        raise SystemExit("unknown case " + case)
    call()
    call()
    wall, dev = [], []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        t0 = time.perf_counter(); call(); wall.append(time.perf_counter() - t0)
        e1.record(stream)
        e1.synchronize()
        dev.append(e0.elapsed_time(e1) * 1e-3)
    ctx.close()
    return {case + "_wall_us": float(np.median(wall)) * 1e6, case + "_device_us": float(np.median(dev)) * 1e6,
            case + "_wall_min_us": float(np.min(wall)) * 1e6, case + "_reps": reps}


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--one":
        print(json.dumps(measure(sys.argv[2], int(sys.argv[3]))))
        return 0
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 50
    path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "computepose_time.json")
    cases = sys.argv[3].split(",") if len(sys.argv) > 3 else CASES
    from ov2slam_amd import _lib as L
    res, rc = {"n_points": N, "p3p_rows": ROWS, "p3p_iterations": ITERS, "library": os.path.relpath(L.LIB_PATH, ROOT)}, 0
    for case in cases:                                                    # one fresh process per case, each under its own limit
        big = case.endswith("4096")
        try:
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", case, str(max(5, reps // 5) if big else reps)],
                                 capture_output=True, text=True, timeout=300 if big else 120)
        except subprocess.TimeoutExpired:
            out = None
        if out is None or out.returncode != 0:
            res[case] = None
            sys.stderr.write("computepose_time: case %s failed%s\n" % (case, "" if out is None else ": " + out.stderr[-2000:]))
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
