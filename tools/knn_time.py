"""Wall time of the loop closer's descriptor matching on the GPU (csrc/knn.hip), host synchronisation included:

    python tools/knn_time.py [reps] [output.json]
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/knn_time.py --one b4096 5     (device time of k_knn per launch;
                                                                  --one SHAPE REPS measures one shape in this process)

Shapes: s308 one item of 308 x 308 rows (an EuRoC keyframe against a loop candidate), s3080 one item of 616 x 3080, b11 a batch
of 11 items of 308 x 308, b4096 a batch of 4096 items of 308 x 308 (8 distinct items repeated).  Prints one JSON line (and writes
it to output.json when given): medians after one warm-up call, in us, of ov2_knn_match / ov2_knn_match_batch.  The ctypes
structures are built once outside the timed region, so the numbers are the C call: host validation, packing into the pinned
staging buffer, one H2D copy, the launches (one, or two when the train rows are split over grid.z), one D2H copy, the host-side
unpacking and pair compaction.  lane_ops is the kernel's arithmetic, n_q * n_t * 25 per item (8 xor, 8 popcount-accumulate, the top-2 update): this is a VALU kernel, its 32 (n_q + n_t)
bytes per item are not what bounds it.  When run as a script each shape is measured by a child process of its own under a time
limit; a shape whose child fails or times out is reported as null and ends the run.
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
SHAPES = {"s308": (0, 308, 308), "s3080": (0, 616, 3080), "b11": (11, 308, 308), "b4096": (4096, 308, 308)}
OPS_PER_PAIR = 25


def median_us(fn, reps):
    fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); t.append(time.perf_counter() - t0)
    return float(np.median(t)) * 1e6


def measure(shape, reps):
    import ov2slam_amd
    from ov2slam_amd import loop_closer as LC
    from ov2slam_amd import _lib as L
    from tests import knn_ref as R
    B, n_q, n_t = SHAPES[shape]
    base = [R.make_case(np.random.default_rng(k), n_q, n_t) for k in range(min(max(B, 1), 8))]
    ctx = ov2slam_amd.Context(0)
    p = LC.knn_params()
    lib = ctx.lib
    n = max(B, 1)
    S = (L.KnnItem * n)()
    Rr = (L.KnnResult * n)()
    keep = {}
    for b in range(n):
        k = b % len(base)
        if k not in keep:
            keep[k] = LC._item(*base[k])
        S[b] = keep[k][0]
        Rr[b], keep[(b, "out")] = LC._result(n_q)
    r = {}
    if B == 0:
        us = median_us(lambda: L.check(lib.ov2_knn_match(ctx.h, C.byref(p), S, Rr)), reps)
        r["%s_wall_us" % shape] = us
        r["%s_pairs" % shape] = int(Rr[0].n_pairs)
    else:
        us = median_us(lambda: L.check(lib.ov2_knn_match_batch(ctx.h, C.byref(p), B, S, Rr)), reps)
        r["%s_wall_us" % shape] = us
        r["%s_wall_us_per_item" % shape] = us / B
    r["%s_lane_ops" % shape] = n * n_q * n_t * OPS_PER_PAIR
    ctx.close()
    return r


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--one":
        print(json.dumps(measure(sys.argv[2], int(sys.argv[3]))))
        return 0
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    res, rc = {}, 0
    for shape in SHAPES:                                                # one fresh process per shape, each under its own limit
        big = SHAPES[shape][0] > 64
        try:
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", shape, str(max(3, reps // 4) if big else reps)],
                                 capture_output=True, text=True, timeout=300 if big else 120)
        except subprocess.TimeoutExpired:
            out = None
        if out is None or out.returncode != 0:
            res["%s_wall_us" % shape] = None
            sys.stderr.write("knn_time: shape %s failed%s\n" % (shape, "" if out is None else ": " + out.stderr[-2000:]))
            rc = 1
            break
        res.update(json.loads(out.stdout.strip().splitlines()[-1]))
    if rc == 0:
        res["b11_over_11_singles"] = res["b11_wall_us"] / (11 * res["s308_wall_us"])
    line = json.dumps(res)
    print(line)
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w") as f:
            f.write(line + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
