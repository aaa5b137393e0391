"""Wall time of the local-map matching on the GPU (csrc/mapmatch.hip), host synchronisation included:

    python tools/match_time.py [reps] [batch sizes, default 11,4096] [output.json]
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/match_time.py --one 11 5     (device time of k_map_match<false> / k_map_pick per
                                                                  launch; --one B REPS measures one size in this process, B = 0: single)

Prints one JSON line (and writes it to output.json when given): medians after one warm-up call, in us, of ov2_match_to_map for one
EuRoC-sized keyframe (3080 local map points, 308 keypoints, about 10 observations and descriptors per map point) and of
ov2_match_to_map_batch for each batch size, made of 8 distinct keyframes repeated.  The ctypes structures are built once outside
the timed region, so the numbers are the C call: host validation, packing into the pinned staging buffer, one H2D copy, the two
launches, one D2H copy, the host-side unpacking.  bytes_per_keyframe is what the call moves per keyframe (every input array once,
every output once); hbm_fraction relates the batch's bytes to its wall time and the 8 TB/s HBM peak of the MI355X -- the wall time
includes the host packing and both PCIe copies, so the fraction is a floor of what the kernels reach (kernel times: the rocprofv3
run).  When run as a script each size is measured by a child process of its own under a time limit; a size whose child fails or
times out is reported as null and ends the run.
"""
import json
import os
import subprocess
import sys
import time

import ctypes as C

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_BYTES_PER_S = 8.0e12


def median_us(fn, reps):
    fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); t.append(time.perf_counter() - t0)
    return float(np.median(t)) * 1e6


def scenes():
    from tests import match_ref as R
    P = R.make_params(D=R.RADTAN4)
    out = []
    for k in range(8):
        M = R.make_scene(P, np.random.default_rng(k), n_kp=270, n_lm=3200, n_kf=20, max_obs=18, dup=0.7)     # + twins: ~308 keypoints
        kf = R.flatten(M)[0]
        n = min(3080, len(kf["lm_mp"]))
        kf["lm_mp"], kf["lm_wpt"] = kf["lm_mp"][:n], kf["lm_wpt"][:n]
        out.append(kf)
    return P, out


def kf_bytes(kf):
    names = ("kp_px", "kp_mp", "cell_start", "cell_kp", "obs_start", "obs_kfid", "obs_kf", "obs_px", "desc_start", "desc", "kf_Tcw",
             "lm_mp", "lm_wpt")
    inp = sum(np.asarray(kf[n]).nbytes for n in names) + 96 + 8 * len(kf["kp_mp"])
    return inp, 17 * len(kf["lm_mp"]) + 8 * len(kf["kp_mp"])


def measure(B, reps):
    import ov2slam_amd
    from ov2slam_amd import mapper
    from ov2slam_amd import _lib as L
    P, base = scenes()
    ctx = ov2slam_amd.Context(0)
    p = mapper._as_match_params(P)
    lib = ctx.lib
    kfs = [base[b % 8] for b in range(max(B, 1))]
    S = (L.MatchKeyframe * len(kfs))()
    Rr = (L.MatchResult * len(kfs))()
    keep = {}
    for b, kf in enumerate(kfs):
        if id(kf) not in keep:
            keep[id(kf)] = mapper._match_keyframe(kf)
        S[b] = keep[id(kf)][0]
        r, out = mapper._match_result(len(kf["lm_mp"]), len(kf["kp_mp"]))
        Rr[b] = r
        keep[(b, "out")] = out
    r = {}
    if B == 0:
        r["single_wall_us"] = median_us(lambda: L.check(lib.ov2_match_to_map(ctx.h, C.byref(p), S, Rr)), reps)
        r["n_lm"], r["n_kp"] = len(kfs[0]["lm_mp"]), len(kfs[0]["kp_mp"])
        r["obs_per_map_point"] = float(np.diff(kfs[0]["obs_start"]).mean())
        r["n_matches"] = int(Rr[0].n_matches)
        h2d, d2h = kf_bytes(kfs[0])
        r["bytes_per_keyframe"] = h2d + d2h
    else:
        us = median_us(lambda: L.check(lib.ov2_match_to_map_batch(ctx.h, C.byref(p), B, S, Rr)), reps)
        nbytes = sum(sum(kf_bytes(kf)) for kf in kfs)
        r["batch%d_wall_us" % B] = us
        r["batch%d_wall_us_per_keyframe" % B] = us / B
        r["batch%d_mb" % B] = nbytes / 1e6
        r["batch%d_hbm_fraction" % B] = nbytes / (us * 1e-6) / HBM_BYTES_PER_S
    ctx.close()
    return r


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--one":
        print(json.dumps(measure(int(sys.argv[2]), int(sys.argv[3]))))
        return 0
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    sizes = [int(v) for v in sys.argv[2].split(",")] if len(sys.argv) > 2 else [11, 4096]
    res, rc = {}, 0
    for B in [0] + sizes:                                               # one fresh process per size, each under its own limit
        n = reps if B <= 64 else max(3, reps // 5)
        try:
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", str(B), str(n)], capture_output=True, text=True,
                                 timeout=120 if B <= 64 else 500)
        except subprocess.TimeoutExpired:
            out = None
        if out is None or out.returncode != 0:
            res["batch%d_wall_us" % B if B else "single_wall_us"] = None
            sys.stderr.write("match_time: size %d failed%s\n" % (B, "" if out is None else ": " + out.stderr[-2000:]))
            rc = 1
            break
        res.update(json.loads(out.stdout.strip().splitlines()[-1]))
    line = json.dumps(res)
    print(line)
    if len(sys.argv) > 3:
        with open(sys.argv[3], "w") as f:
            f.write(line + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
