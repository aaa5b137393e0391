#!/usr/bin/env python3
"""What device rectification (ov2_rectify_*, ov2_*_set_rectification; csrc/rectify.hip) costs, and that the unrectified forms cost
what they did before it existed.

    rectify_time.py [--batch 4096] [--reps 9] [--parent-lib PATH] [--out profiles/rectify_time.json]

Measured at 752 x 480 with a EuRoC-like map (tests/remap_ref.py):
  rectify_h            ov2_rectify_h, host in / host out, wall clock per call (synchronising)
  track_frame[_rect]   ov2_tracker_track_frame with the ~270 keypoints of a 35-pixel grid (graph replay), wall clock per call, without / with the map set
  step[_rect]          the lock-step pre-processing of `batch` device-resident frames (ov2_pyr_build_clahe_d), HIP events, without /
                       with ov2_rectify_d in front of it; rectify_d: that launch alone
Every figure is the median of --reps repetitions after a warm-up.  With --parent-lib (a build of the parent commit's library) the
unrectified forms are measured on that build too, in the same session, alternating parent / new / parent / new in fresh processes:
the new build's unrectified medians are reported next to the parent's own run-to-run spread.  --worker runs one such process."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
W, H = 752, 480
RECT_SYMBOLS = ("ov2_rectmap_create", "ov2_rectmap_destroy", "ov2_rectify_h", "ov2_rectify_d", "ov2_pyr_build_rect_h",
                "ov2_tracker_set_rectification", "ov2_btracker_set_rectification")


def _stats(ms):
    s = sorted(ms)
    return {"median_ms": s[len(s) // 2], "min_ms": s[0], "max_ms": s[-1], "reps": len(s)}


def worker(batch, reps, baseline):
    import numpy as np
    import torch
    torch.cuda.init()                      # torch's HIP runtime must be initialised before libov2slam_hip.so in one process
    from ov2slam_amd import _lib as L
    if baseline:                           # a library from before the rectification symbols: bind what it has
        for s in RECT_SYMBOLS:
            L.SIGNATURES.pop(s, None)
    import ov2slam_amd
    from ov2slam_amd import synth
    from tests import remap_ref as R
    from tests.test_gpu_tracker import _sequence, _points

    res = {}
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream()
    ctx = ov2slam_amd.Context(0, stream=stream.cuda_stream)       # the batch part: torch's stream, timed with its events
    own = ov2slam_amd.Context(0)                                  # the single-image parts: a stream the tracker can capture
    maps = R.both_forms(*R.euroc_like_maps(W, H))
    rm = None if baseline else ov2slam_amd.RectifyMap(ctx, "fixed", *maps["fixed"])
    rm_own = None if baseline else ov2slam_amd.RectifyMap(own, "fixed", *maps["fixed"])

    # ---- single image, host in / host out
    frames, flow = _sequence(W, H, 2, seed=5)
    if rm is not None:
        out = np.empty((H, W), np.uint8)
        ts = []
        for r in range(reps + 3):
            t0 = time.perf_counter(); rm_own.rectify(frames[r & 1], out=out); ts.append((time.perf_counter() - t0) * 1e3)
        res["rectify_h"] = _stats(ts[3:])

    # ---- the per-frame call of the single tracker
    rng = np.random.default_rng(1)
    k, p, hp = _points(W, H, flow, 0, rng, 1.0)
    k, p, hp = k[:300], p[:300], hp[:300]
    empty = np.zeros((0, 2), np.float32)
    for name, use in (("track_frame", None), ("track_frame_rect", rm_own)):
        if name.endswith("_rect") and rm is None:
            continue
        t = ov2slam_amd.VisualFrontEndTracker(own, W, H, nbmaxkps=512)
        if use is not None:
            t.setRectification(use)
        t.image_buffer[:, :W] = frames[0]
        t.trackFrame(t.image_buffer, empty, empty, None)
        res.setdefault("uses_graph", bool(t.uses_graph))
        ts = []
        for r in range(5 * reps + 5):
            t.image_buffer[:, :W] = frames[(r + 1) & 1]
            t0 = time.perf_counter(); t.trackFrame(t.image_buffer, k, p, hp); ts.append((time.perf_counter() - t0) * 1e3)
        res[name] = _stats(ts[5:])
        t.close()

    # ---- lock-step pre-processing of `batch` resident frames
    views = np.stack([synth.frame_pair(W, H, seed=40 + s)[0] for s in range(8)])
    fr = torch.from_numpy(views).to(dev)[torch.arange(batch, device=dev) % 8].contiguous()
    P = ov2slam_amd.Pyramid(ctx, W, H, 9, 3, batch=batch)
    rect = torch.empty_like(fr) if rm is not None else None

    def timed(fn):
        ts = []
        for r in range(reps + 2):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream); fn(); e1.record(stream); torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        return _stats(ts[2:])

    res["step"] = timed(lambda: P.build_clahe_from_device(fr.data_ptr(), 3.0, W // 50, H // 50))
    if rm is not None:
        remap = lambda: rm.rectify_device(fr.data_ptr(), W, W * H, batch, rect.data_ptr(), W, W * H)
        res["rectify_d"] = timed(remap)
        res["step_rect"] = timed(lambda: (remap(), P.build_clahe_from_device(rect.data_ptr(), 3.0, W // 50, H // 50)))
        res["step_again"] = timed(lambda: P.build_clahe_from_device(fr.data_ptr(), 3.0, W // 50, H // 50))
    P.close()
    own.close()
    ctx.close()
    print("RECTIFY_TIME " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rectify_time.json"))
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--baseline", action="store_true")
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps must be at least 5")
    if a.worker:
        return worker(a.batch, a.reps, a.baseline)

    def run(lib, baseline):
        env = dict(os.environ)
        if lib:
            env["OV2SLAM_HIP_LIB"] = lib
        cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--batch", str(a.batch), "--reps", str(a.reps)] + (["--baseline"] if baseline else [])
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
        line = [l for l in r.stdout.splitlines() if l.startswith("RECTIFY_TIME ")]
        if r.returncode != 0 or not line:
            raise SystemExit("worker failed (%s):\n%s" % (lib or "this build", r.stderr[-3000:]))
        return json.loads(line[0][len("RECTIFY_TIME "):])

    order = ["parent", "new", "parent", "new"] if a.parent_lib else ["new"]
    runs = [{"build": b, "measures": run(a.parent_lib if b == "parent" else None, b == "parent")} for b in order]
    frame_bytes = W * H
    out = {"size": [W, H], "batch": a.batch, "reps": a.reps, "runs": runs,
           "byte_bound": {"read_plus_write_bytes_per_step": 2 * frame_bytes * a.batch,
                          "ms_at_8_TB_per_s": 2 * frame_bytes * a.batch / 8e12 * 1e3}}
    new = [r["measures"] for r in runs if r["build"] == "new"]
    med = lambda rs, key: sorted(r[key]["median_ms"] for r in rs)[len(rs) // 2]
    summary = {key: med(new, key) for key in new[0] if key != "uses_graph"}
    summary["step_extra_ms"] = summary["step_rect"] - summary["step"]
    summary["track_frame_extra_ms"] = summary["track_frame_rect"] - summary["track_frame"]
    if a.parent_lib:
        par = [r["measures"] for r in runs if r["build"] == "parent"]
        cmp_ = {}
        for key in ("track_frame", "step"):
            lo = min(r[key]["min_ms"] for r in par); hi = max(r[key]["max_ms"] for r in par)
            cmp_[key] = {"parent_medians_ms": [r[key]["median_ms"] for r in par], "parent_min_ms": lo, "parent_max_ms": hi,
                         "new_medians_ms": [r[key]["median_ms"] for r in new],
                         "new_within_parent_spread": all(lo <= r[key]["median_ms"] <= hi for r in new)}
        summary["unrectified_vs_parent"] = cmp_
    out["summary"] = summary
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(summary, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
