"""Wall time of the keyframe triangulation on the GPU (csrc/triangulate.hip), host synchronisation included:

    python tools/tri_time.py [reps]
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/tri_time.py     (device time of k_triangulate per launch)

Prints one JSON line: us of wall time of ov2_triangulate_keyframe for one 308-point keyframe (EuRoC-like unrectified stereo pair,
5 source keyframes) and of ov2_triangulate_keyframe_batch for 11 and 4096 such keyframes.  The ctypes structures are built once
outside the timed region, so the numbers are the C call: host validation and packing into the pinned staging buffer, one H2D
copy, the launch, one D2H copy, the host-side unpacking.  h2d_mb / d2h_mb are the bytes each batch moves.
"""
import json
import os
import sys
import time

import ctypes as C

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def best(fn, reps):
    fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); t.append(time.perf_counter() - t0)
    return float(np.median(t)) * 1e6


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    import ov2slam_amd
    from ov2slam_amd import mapper
    from ov2slam_amd import _lib as L
    from tests import tri_ref as R
    ctx = ov2slam_amd.Context(0)
    P = R.make_params(R.EUROC, stereo=True, rect=False, seed=1)
    base = []
    for k in range(8):
        M = R.make_map(P, np.random.default_rng(k), n=308, n_src=5, noise=0.2, behind=0.02)
        base.append(R.inputs_from_map(M)[0])
    p = mapper._as_params(P)
    lib = ctx.lib

    def prepared(kfs):
        S = (L.TriKeyframe * len(kfs))()
        Rr = (L.TriResult * len(kfs))()
        keep = []
        for b, kf in enumerate(kfs):
            s, k, n = mapper._keyframe(kf)
            r, out = mapper._result(n)
            S[b], Rr[b] = s, r
            keep.append((k, out))
        return S, Rr, keep

    r = {}
    S1, R1, k1 = prepared(base[:1])
    r["single_308_wall_us"] = best(lambda: L.check(lib.ov2_triangulate_keyframe(ctx.h, C.byref(p), S1, R1)), reps)
    for B in (11, 4096):
        SB, RB, kB = prepared([base[b % 8] for b in range(B)])
        r["batch%d_wall_us" % B] = best(lambda: L.check(lib.ov2_triangulate_keyframe_batch(ctx.h, C.byref(p), B, SB, RB)), reps)
        r["batch%d_h2d_mb" % B] = B * (308 * 101 + 16 + 56 + 5 * 112) / 1e6
        r["batch%d_d2h_mb" % B] = B * 308 * 33 / 1e6
    ctx.close()
    print(json.dumps(r))


if __name__ == "__main__":
    main()
