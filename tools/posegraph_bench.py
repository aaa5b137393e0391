#!/usr/bin/env python3
"""Times the device pose-graph solver (ov2_pose_graph_solve) on the shapes DESIGN.md 4.12 records: localPoseGraph over one segment of
64, 257 and 1500 keyframes, fullPoseGraph over 2000 frames with a keyframe every 10, a batch of 64 localPoseGraph problems of 65
keyframes, and the apply step.  Prints one JSON line per shape: device time of the launch (solve_ms, HIP events) and wall time of
the call, best of --repeat.  The scenes are those of tests/posegraph_ref.py; nothing is checked here (tests/test_gpu_posegraph.py does)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=5)
    a = ap.parse_args()
    import ov2slam_amd
    from ov2slam_amd import optimizer as O
    from tests import posegraph_ref as R
    ctx = ov2slam_amd.Context(0)

    def best(fn):
        out, ms, wall = None, float("inf"), float("inf")
        for _ in range(a.repeat + 1):                       # the first call grows the context's buffers
            t = time.perf_counter(); out = fn(); w = 1e3 * (time.perf_counter() - t)
            one = out[0] if isinstance(out, list) else out
            ms, wall = min(ms, one["solve_ms"]), min(wall, w)
        return out, ms, wall

    for n in (64, 257, 1500):
        p = R.make_local_scene(np.random.default_rng(100 + n), n)
        out, ms, wall = best(lambda: O.pose_graph(ctx, p))
        print(json.dumps(dict(shape="localPoseGraph", poses=n, segments=1, iterations=out["iterations"], termination=out["termination"],
                              solve_ms=round(ms, 4), ms_per_iteration=round(ms / max(1, out["iterations"]), 4), wall_ms=round(wall, 4))))
    p = R.make_full_scene(np.random.default_rng(2000), 2000, 10)
    opts = O.pose_graph_options(ctx.lib, full=True)
    out, ms, wall = best(lambda: O.pose_graph(ctx, p, opts))
    print(json.dumps(dict(shape="fullPoseGraph", poses=2000, segments=len(R.Structure(p).segments), iterations=out["iterations"],
                          termination=out["termination"], solve_ms=round(ms, 4), ms_per_iteration=round(ms / max(1, out["iterations"]), 4),
                          wall_ms=round(wall, 4))))
    probs = [R.make_local_scene(np.random.default_rng(500 + i), 65) for i in range(64)]
    out, ms, wall = best(lambda: O.pose_graph_batch(ctx, probs))
    print(json.dumps(dict(shape="localPoseGraph batch", items=64, poses=65, iterations=[o["iterations"] for o in out][:4], solve_ms=round(ms, 4),
                          wall_ms=round(wall, 4))))
    rng = np.random.default_rng(1)
    P = R.arc(1030)
    X = rng.normal(0, 20, (200000, 3)); kf = rng.integers(0, 1030, 200000).astype(np.int32)
    wall = float("inf")
    for _ in range(a.repeat + 1):
        t = time.perf_counter(); O.pose_graph_apply(ctx, P[:1000], P[:1000], R.inv_pose(P[999]), P[999], P[1000:], X, kf)
        wall = min(wall, 1e3 * (time.perf_counter() - t))
    print(json.dumps(dict(shape="apply", window=1000, young=30, points=200000, wall_ms=round(wall, 4))))
    ctx.close()


if __name__ == "__main__":
    main()
