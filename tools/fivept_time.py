"""Wall and device time of the 5-point essential-matrix search on the GPU (csrc/fivept.hip):

    python tools/fivept_time.py [reps] [output.json, default profiles/fivept_time.json]
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/fivept_time.py --one 11 200 5       (per-kernel times of one case)

Prints one JSON line (and writes it): medians after one warm-up call, in us, for
    front end      one 308-match problem (0.5 px noise, 30 % outliers), 100 iterations over 200 rows
    batches        11 and 4096 problems of that kind (8 distinct scenes repeated)
wall = the C call (host validation, packing, one H2D copy, three launches, one D2H copy, unpacking); device = the time between two
events on the context's stream around the call, i.e. both copies and the three kernels.  Times only: the host loop of the reference
runs inside OpenGV, which is not available to this project, so there is no baseline and NO SPEED-UP IS CLAIMED.  Each case runs in
a child process of its own under a time limit; a case whose child fails or times out is reported as null and ends the run."""
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CASES = [(0, 200), (11, 200), (4096, 200)]


def measure(B, rows, reps):
    import torch
    import ov2slam_amd
    from ov2slam_amd import pose
    from ov2slam_amd import _lib as L
    from tests import fivept_ref as R
    stream = torch.cuda.Stream()
    ctx = ov2slam_amd.Context(0, stream=stream.cuda_stream)
    n = 308
    base = []
    for k in range(8):
        bv1, bv2, _, _, _ = R.make_scene(np.random.default_rng(k), n, noise_px=0.5, outlier_frac=0.3)
        base.append(dict(bv1=bv1, bv2=bv2, samples=pose.epipolar_draw_samples(k, n, rows)))
    nb = max(B, 1)
    S, Rr, keep = (L.EpipolarProblem * nb)(), (L.EpipolarResult * nb)(), []
    for b in range(nb):
        S[b], Rr[b], k = pose._epi_problem(base[b % 8], False)
        keep.append(k)
    P = pose.epipolar_params(rows // 2, R.threshold_of(3.0, 460.0, 460.0))
    if B == 0:
        call = lambda: L.check(ctx.lib.ov2_epipolar_ransac(ctx.h, C.byref(P), S, Rr))
    else:
        call = lambda: L.check(ctx.lib.ov2_epipolar_ransac_batch(ctx.h, C.byref(P), B, S, Rr))
    call()
    wall, dev = [], []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        t0 = time.perf_counter(); call(); wall.append(time.perf_counter() - t0)
        e1.record(stream)
        e1.synchronize()
        dev.append(e0.elapsed_time(e1) * 1e-3)
    name = ("single_%drows" % rows) if B == 0 else ("batch%d_%drows" % (B, rows))
    r = {name + "_wall_us": float(np.median(wall)) * 1e6, name + "_device_us": float(np.median(dev)) * 1e6,
         name + "_iterations": int(Rr[0].iterations), name + "_inliers": int(Rr[0].n_inliers), name + "_status": int(Rr[0].status)}
    ctx.close()
    return r


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--one":
        print(json.dumps(measure(int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]))))
        return 0
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "fivept_time.json")
    res, rc = {"n_points": 308}, 0
    for B, rows in CASES:                                                 # one fresh process per case, each under its own limit
        n = reps if B <= 64 else max(3, reps // 5)
        try:
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", str(B), str(rows), str(n)],
                                 capture_output=True, text=True, timeout=120 if B <= 64 else 400)
        except subprocess.TimeoutExpired:
            out = None
        if out is None or out.returncode != 0:
            res["%d_%d" % (B, rows)] = None
            sys.stderr.write("fivept_time: case %d %d failed%s\n" % (B, rows, "" if out is None else ": " + out.stderr[-2000:]))
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
