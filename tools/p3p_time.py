"""Wall and device time of the P3P pose search on the GPU (csrc/p3p.hip):

    python tools/p3p_time.py [reps] [output.json, default profiles/p3p_time.json]
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/p3p_time.py --one lmeds 11 200 5     (per-kernel times of one case)

Prints one JSON line (and writes it): medians after one warm-up call, in us, for
    front end      one 308-point problem (0.5 px noise, 30 % outliers), LMedS, 100 iterations over 200 rows
    loop closer    the same problem, RANSAC, 1000 iterations over 2000 rows
    batches        11 and 4096 problems of the front-end kind (8 distinct scenes repeated), LMedS
wall = the C call (host validation, packing, one H2D copy, three launches, one D2H copy, unpacking); device = the time between two
events on the context's stream around the call, i.e. both copies and the three kernels.  Times only: OpenGV is not available to
this project, so there is no baseline to compare with.  Each case runs in a child process of its own under a time limit; a case
whose child fails or times out is reported as null and ends the run."""
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CASES = [("lmeds", 0, 200), ("ransac", 0, 2000), ("lmeds", 11, 200), ("lmeds", 4096, 200)]


def measure(mode, B, rows, reps):
    import torch
    import ov2slam_amd
    from ov2slam_amd import pose
    from ov2slam_amd import _lib as L
    from tests import p3p_ref as R
    stream = torch.cuda.Stream()
    ctx = ov2slam_amd.Context(0, stream=stream.cuda_stream)
    n = 308
    base = []
    for k in range(8):
        bv, X, _, _, _ = R.make_scene(np.random.default_rng(k), n, noise_px=0.5, outlier_frac=0.3)
        base.append(dict(bv=bv, X=X, samples=pose.draw_samples(k, n, rows)))
    nb = max(B, 1)
    S, Rr, keep = (L.P3PProblem * nb)(), (L.P3PResult * nb)(), []
    for b in range(nb):
        S[b], Rr[b], k = pose._problem(base[b % 8], False)
        keep.append(k)
    P = pose.p3p_params(pose.LMEDS if mode == "lmeds" else pose.RANSAC, rows // 2, R.threshold_of(3.0, 460.0, 460.0))
    if B == 0:
        call = lambda: L.check(ctx.lib.ov2_p3p_ransac(ctx.h, C.byref(P), S, Rr))
    else:
        call = lambda: L.check(ctx.lib.ov2_p3p_ransac_batch(ctx.h, C.byref(P), B, S, Rr))
    call()
    wall, dev = [], []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        t0 = time.perf_counter(); call(); wall.append(time.perf_counter() - t0)
        e1.record(stream)
        e1.synchronize()
        dev.append(e0.elapsed_time(e1) * 1e-3)
    name = ("single_%s_%drows" % (mode, rows)) if B == 0 else ("batch%d_%s_%drows" % (B, mode, rows))
    r = {name + "_wall_us": float(np.median(wall)) * 1e6, name + "_device_us": float(np.median(dev)) * 1e6,
         name + "_iterations": int(Rr[0].iterations), name + "_inliers": int(Rr[0].n_inliers), name + "_status": int(Rr[0].status)}
    ctx.close()
    return r


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--one":
        print(json.dumps(measure(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5]))))
        return 0
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "p3p_time.json")
    res, rc = {"n_points": 308}, 0
    for mode, B, rows in CASES:                                           # one fresh process per case, each under its own limit
        n = reps if B <= 64 else max(3, reps // 5)
        try:
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", mode, str(B), str(rows), str(n)],
                                 capture_output=True, text=True, timeout=120 if B <= 64 else 400)
        except subprocess.TimeoutExpired:
            out = None
        if out is None or out.returncode != 0:
            res["%s_%d_%d" % (mode, B, rows)] = None
            sys.stderr.write("p3p_time: case %s %d %d failed%s\n" % (mode, B, rows, "" if out is None else ": " + out.stderr[-2000:]))
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
