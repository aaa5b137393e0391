"""Wall time of the tracking priors on the GPU (csrc/priors.hip), host synchronisation included:

    python tools/priors_time.py [reps]
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/priors_time.py     (device time of k_prior_frame / k_prior_stereo per launch)

Prints one JSON line: us of wall time of ov2_klt_priors and ov2_stereo_priors (unrectified: the neighbour branch runs) for one
EuRoC-sized item (308 keypoints, radtan distortion), of the batch forms for 11 and 4096 such items, and of 11 single calls in the same
run.  The ctypes structures are built once outside the timed region, so the numbers are the C call: host validation (the cell
tables included) and packing into the pinned staging buffer, one H2D copy, the launch, one D2H copy, the host-side unpacking.
*_bytes_per_item are the algorithmic bytes: every input array the form reads once plus its outputs; *_us_at_8tbs is what one read
plus one write of them would take at 8 TB/s.
"""
import json
import os
import sys
import time

import ctypes as C

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N = 308
NCELLS = 22 * 14
# ov2_klt_priors: item 16 + Tcw 56, px 8 + wpt 24 + is3d 1 per keypoint in, prior 8 + has_prior 1 out
KLT_BYTES = 16 + 56 + N * (8 + 24 + 1) + N * (8 + 1)
# ov2_stereo_priors: item 16 + Tcw 56, px 8 + unpx 8 + bv 24 + wpt 24 + state 1 per keypoint, cell_start 4 per cell + 1, cell_kp 4 per
# keypoint in, prior 8 + has_prior 1 + skip 1 out
STEREO_BYTES = 16 + 56 + N * (8 + 8 + 24 + 24 + 1) + 4 * (NCELLS + 1) + 4 * N + N * (8 + 1 + 1)


def best(fn, reps):
    fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); t.append(time.perf_counter() - t0)
    return float(np.median(t)) * 1e6


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    import ov2slam_amd
    from ov2slam_amd import priors as PR
    from ov2slam_amd import _lib as L
    from tests import priors_ref as R
    ctx = ov2slam_amd.Context(0)
    P = R.make_params(D=R.RADTAN4, klt_use_prior=True, rect=False)
    base = [R.flatten(P, *R.make_scene(P, np.random.default_rng(k), N)) for k in range(8)]
    pk, ps = PR._as_klt_params(P), PR._as_stereo_params(P)
    lib = ctx.lib

    def prepared(items):
        SK, RK = (L.KltPriorsItem * len(items))(), (L.KltPriorsResult * len(items))()
        SS, RS = (L.StereoPriorsItem * len(items))(), (L.StereoPriorsResult * len(items))()
        keep = []
        for b, it in enumerate(items):
            SK[b], k1 = PR._klt_item(it)
            SS[b], k2 = PR._stereo_item(it)
            RK[b], o1 = PR._klt_result(SK[b].n)
            RS[b], o2 = PR._stereo_result(SS[b].n)
            keep.append((k1, k2, o1, o2))
        return SK, RK, SS, RS, keep

    r = {}
    SK, RK, SS, RS, k1 = prepared(base[:1])
    r["klt_single_wall_us"] = best(lambda: L.check(lib.ov2_klt_priors(ctx.h, C.byref(pk), SK, RK)), reps)
    r["stereo_single_wall_us"] = best(lambda: L.check(lib.ov2_stereo_priors(ctx.h, C.byref(ps), SS, RS)), reps)
    r["klt_prior_share"] = RK[0].n_prior / N
    r["stereo_prior3d_share"], r["stereo_prior_nb_share"] = RS[0].n_prior3d / N, RS[0].n_prior_nb / N
    singles = [prepared([base[b % 8]]) for b in range(11)]

    def eleven_klt():
        for sk, rk, ss, rs, k in singles:
            L.check(lib.ov2_klt_priors(ctx.h, C.byref(pk), sk, rk))

    def eleven_stereo():
        for sk, rk, ss, rs, k in singles:
            L.check(lib.ov2_stereo_priors(ctx.h, C.byref(ps), ss, rs))
    r["klt_11_singles_wall_us"] = best(eleven_klt, reps)
    r["stereo_11_singles_wall_us"] = best(eleven_stereo, reps)
    for B in (11, 4096):
        SKB, RKB, SSB, RSB, kB = prepared([base[b % 8] for b in range(B)])
        r["klt_batch%d_wall_us" % B] = best(lambda: L.check(lib.ov2_klt_priors_batch(ctx.h, C.byref(pk), B, SKB, RKB)), reps)
        r["stereo_batch%d_wall_us" % B] = best(lambda: L.check(lib.ov2_stereo_priors_batch(ctx.h, C.byref(ps), B, SSB, RSB)), reps)
    r["klt_bytes_per_item"], r["stereo_bytes_per_item"] = KLT_BYTES, STEREO_BYTES
    r["klt_batch4096_us_at_8tbs"] = 4096 * KLT_BYTES / 8e12 * 1e6
    r["stereo_batch4096_us_at_8tbs"] = 4096 * STEREO_BYTES / 8e12 * 1e6
    ctx.close()
    print(json.dumps(r))


if __name__ == "__main__":
    main()
