"""Wall time of the frame-versus-keyframe passes on the GPU (csrc/fkf.hip), host synchronisation included:

    python tools/kfreq_time.py [reps]
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/kfreq_time.py     (device time of k_fkf_parallax / k_fkf_sampson per launch)

Prints one JSON line: us of wall time of ov2_kf_decision (counts taken on the device) and ov2_sampson_filter_2d for one EuRoC-sized
item (308 current keypoints against a 308-keypoint keyframe, 80 % of them known to it), of the batch forms for 11 and 4096 such
items, and of 11 single calls in the same run.  The ctypes structures are built once outside the timed region, so the numbers are
the C call: host validation (the ascending-id check included) and packing into the pinned staging buffer, one H2D copy, the launch,
one D2H copy, the host-side unpacking.  *_bytes_per_item are the algorithmic bytes: every input array the form reads once plus the
result record; *_us_at_8tbs is what moving them once would take at 8 TB/s.
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
# ov2_kf_decision, counted: item header 176, cur_lmid 4 + cur_px 8 + cur_bv 24 + cur_is3d 1 per current keypoint, kf_lmid 4 + kf_unpx 8
# per keyframe keypoint, a 36-byte record back
DECISION_BYTES = 176 + N * (4 + 8 + 24 + 1) + N * (4 + 8) + 36
# ov2_sampson_filter_2d: header 176 + F 72, cur_lmid 4 + cur_unpx 8 + cur_is3d 1, kf_lmid 4 + kf_unpx 8, err 4 + bad 1 back
SAMPSON_BYTES = 176 + 72 + N * (4 + 8 + 1) + N * (4 + 8) + N * (4 + 1)


def best(fn, reps):
    fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); t.append(time.perf_counter() - t0)
    return float(np.median(t)) * 1e6


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    import ov2slam_amd
    from ov2slam_amd import keyframe as KF
    from ov2slam_amd import _lib as L
    from tests import kfreq_ref as R
    ctx = ov2slam_amd.Context(0)
    P = R.make_params(stereo=True)
    base = [R.flatten(*R.make_scene(P, np.random.default_rng(k), N, N, known=0.8)) for k in range(8)]
    p = KF._as_fkf_params(P)
    F = np.tile(R.make_F(np.random.default_rng(0)), (4096, 1))
    Fp = F.ctypes.data_as(C.POINTER(C.c_double))
    lib = ctx.lib

    def prepared(items):
        S = (L.FkfItem * len(items))()
        D = (L.KfDecisionResult * len(items))()
        Sr = (L.Sampson2dResult * len(items))()
        keep = []
        for b, it in enumerate(items):
            S[b], k = KF._fkf_item(it)
            Sr[b], out = KF._sampson_result(S[b].n_cur)
            keep.append((k, out))
        return S, D, Sr, keep

    r = {}
    S1, D1, Sr1, k1 = prepared(base[:1])
    r["decision_single_wall_us"] = best(lambda: L.check(lib.ov2_kf_decision(ctx.h, C.byref(p), S1, D1)), reps)
    r["sampson_single_wall_us"] = best(lambda: L.check(lib.ov2_sampson_filter_2d(ctx.h, S1, Fp, 3.0, Sr1)), reps)
    singles = [prepared([base[b % 8]]) for b in range(11)]

    def eleven_decisions():
        for S, D, Sr, k in singles:
            L.check(lib.ov2_kf_decision(ctx.h, C.byref(p), S, D))

    def eleven_sampsons():
        for S, D, Sr, k in singles:
            L.check(lib.ov2_sampson_filter_2d(ctx.h, S, Fp, 3.0, Sr))
    r["decision_11_singles_wall_us"] = best(eleven_decisions, reps)
    r["sampson_11_singles_wall_us"] = best(eleven_sampsons, reps)
    for B in (11, 4096):
        SB, DB, SrB, kB = prepared([base[b % 8] for b in range(B)])
        r["decision_batch%d_wall_us" % B] = best(lambda: L.check(lib.ov2_kf_decision_batch(ctx.h, C.byref(p), B, SB, DB)), reps)
        r["sampson_batch%d_wall_us" % B] = best(lambda: L.check(lib.ov2_sampson_filter_2d_batch(ctx.h, B, SB, Fp, 3.0, SrB)), reps)
    r["decision_bytes_per_item"], r["sampson_bytes_per_item"] = DECISION_BYTES, SAMPSON_BYTES
    r["decision_batch4096_us_at_8tbs"] = 4096 * DECISION_BYTES / 8e12 * 1e6
    r["sampson_batch4096_us_at_8tbs"] = 4096 * SAMPSON_BYTES / 8e12 * 1e6
    ctx.close()
    print(json.dumps(r))


if __name__ == "__main__":
    main()
