"""Wall time of the loop local-map tracking on the GPU (csrc/mapmatch.hip), host synchronisation included:

    python tools/loopmap_time.py [reps] [batch sizes, default 11,4096] [output.json]
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/loopmap_time.py --one 11 5   (device time of k_map_match<true> / k_map_pick
                                                                  per launch; --one B REPS measures one size in this process, B = 0:
                                                                  single, B = -1: ov2_match_to_map on the same scene)

Prints one JSON line (and writes it to output.json when given): medians after one warm-up call, in us, of ov2_loop_match_to_map for
one EuRoC-sized loop candidate (3080 local map points, about 308 keypoints of which about 100 are flagged matched, about 9
observations and descriptors per map point, radial-tangential calibration) and of ov2_loop_match_to_map_batch for each batch size,
made of 8 distinct candidates repeated.  The ctypes structures are built once outside the timed region, so the numbers are the C
call: host validation, packing into the pinned staging buffer, one H2D copy, the two launches, one D2H copy, the host-side
unpacking.  It also reports
  - survivors_per_point: keypoints that pass the lane-local gates (matched flag, usable map point, 10 px) per local map point that
    projects into the image, and compared_per_point: those that also pass the shared-observer test, counted by the numpy
    specification on the first candidate (no GPU involved);
  - the two relations that need no outside number: batch11_below_11_singles (the batch of 11 costs less wall time than 11 single
    calls) and, when 4096 was measured, batch4096_per_item_below_single (wall time per item; the kernels' own time per item comes
    from the rocprofv3 run above);
  - match_to_map_wall_us, for orientation only: ov2_match_to_map (the mapper's loop: 2 px gate, re-projection gate) on the scene
    the candidate was made from.
When run as a script each size is measured by a child process of its own under a time limit; a size whose child fails or times out
is reported as null and ends the run.
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
SCENE = dict(n_kp=270, n_lm=3600, n_kf=20, max_obs=18, dup=0.7)        # + twins: ~308 keypoints; trimmed to 3080 local map points


def median_us(fn, reps):
    fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); t.append(time.perf_counter() - t0)
    return float(np.median(t)) * 1e6


def scenes(n=8):
    from tests import loopmap_ref as R
    P = R.make_params(D=R.RADTAN4)
    out = []
    for k in range(n):
        M = R.make_scene(P, np.random.default_rng(k), matched=0.25, **SCENE)
        item, meta = R.flatten(M)
        out.append(R.trim(item, meta, 3080)[0])
    return P, out


def mapper_scene():
    """the mapper's view of the scene candidate 0 was made from (the generator draws it first, from the same seed)"""
    from tests import match_ref as MR
    P = MR.make_params(D=MR.RADTAN4)
    kf = MR.flatten(MR.make_scene(P, np.random.default_rng(0), **SCENE))[0]
    n = min(3080, len(kf["lm_mp"]))
    kf["lm_mp"], kf["lm_wpt"] = kf["lm_mp"][:n], kf["lm_wpt"][:n]
    return P, kf


def survivors():
    from tests import loopmap_ref as R
    P, items = scenes(1)
    ev = {}
    R.flat(P, items[0], ev)
    n = max(ev.get("in_image", 0), 1)
    return dict(points_in_image=ev.get("in_image", 0), block_keypoints_per_point=ev.get("block_kp", 0) / n,
                survivors_per_point=ev.get("survivors", 0) / n, compared_per_point=ev.get("compared", 0) / n)


def measure(B, reps):
    import ov2slam_amd
    from ov2slam_amd import _lib as L
    ctx = ov2slam_amd.Context(0)
    lib = ctx.lib
    r = {}
    if B < 0:
        from ov2slam_amd import mapper
        P, kf = mapper_scene()
        p = mapper._as_match_params(P)
        s, keep, n_lm, n_kp = mapper._match_keyframe(kf)
        res, out = mapper._match_result(n_lm, n_kp)
        r["match_to_map_wall_us"] = median_us(lambda: L.check(lib.ov2_match_to_map(ctx.h, C.byref(p), C.byref(s), C.byref(res))), reps)
        r["match_to_map_n_lm"], r["match_to_map_n_kp"], r["match_to_map_n_matches"] = n_lm, n_kp, int(res.n_matches)
        ctx.close()
        return r
    from ov2slam_amd import loop_closer as LC
    P, base = scenes()
    p = LC._as_loopmap_params(P)
    items = [base[b % 8] for b in range(max(B, 1))]
    S = (L.LoopMapItem * len(items))()
    Rr = (L.LoopMapResult * len(items))()
    keep = {}
    for b, item in enumerate(items):
        if id(item) not in keep:
            keep[id(item)] = LC._loopmap_item(item)
        S[b] = keep[id(item)][0]
        res, out = LC._loopmap_result(len(item["lm_mp"]), len(item["kp_mp"]))
        Rr[b] = res
        keep[(b, "out")] = out
    if B == 0:
        r["single_wall_us"] = median_us(lambda: L.check(lib.ov2_loop_match_to_map(ctx.h, C.byref(p), S, Rr)), reps)
        r["n_lm"], r["n_kp"], r["n_kp_matched"] = len(items[0]["lm_mp"]), len(items[0]["kp_mp"]), int(items[0]["kp_matched"].sum())
        r["obs_per_map_point"] = float(np.diff(items[0]["obs_start"]).mean())
        r["n_matches"] = int(Rr[0].n_matches)
    else:
        us = median_us(lambda: L.check(lib.ov2_loop_match_to_map_batch(ctx.h, C.byref(p), B, S, Rr)), reps)
        r["batch%d_wall_us" % B] = us
        r["batch%d_wall_us_per_item" % B] = us / B
    ctx.close()
    return r


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--one":
        print(json.dumps(measure(int(sys.argv[2]), int(sys.argv[3]))))
        return 0
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    sizes = [int(v) for v in sys.argv[2].split(",")] if len(sys.argv) > 2 else [11, 4096]
    res, rc = survivors(), 0
    for B in [0] + sizes + [-1]:                                        # one fresh process per size, each under its own limit
        n = reps if B <= 64 else max(3, reps // 5)
        try:
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", str(B), str(n)], capture_output=True, text=True,
                                 timeout=120 if B <= 64 else 500)
        except subprocess.TimeoutExpired:
            out = None
        if out is None or out.returncode != 0:
            res["batch%d_wall_us" % B if B > 0 else ("single_wall_us" if B == 0 else "match_to_map_wall_us")] = None
            sys.stderr.write("loopmap_time: size %d failed%s\n" % (B, "" if out is None else ": " + out.stderr[-2000:]))
            rc = 1
            break
        res.update(json.loads(out.stdout.strip().splitlines()[-1]))
    single = res.get("single_wall_us")
    if single and res.get("batch11_wall_us"):
        res["batch11_below_11_singles"] = bool(res["batch11_wall_us"] < 11 * single)
    if single and res.get("batch4096_wall_us"):
        res["batch4096_per_item_below_single"] = bool(res["batch4096_wall_us_per_item"] < single)
    line = json.dumps(res)
    print(line)
    if len(sys.argv) > 3:
        with open(sys.argv[3], "w") as f:
            f.write(line + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
