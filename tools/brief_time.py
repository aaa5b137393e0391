"""describeBRIEF timings on the GPU (csrc/brief.hip), each the median of --reps runs after warm-up, host clock around calls that end
in a device synchronisation:
  host      ov2_describe_brief on a EuRoC keyframe (752 x 480, 616 points = the frame's existing + new keypoints), H2D and sync included
  tracker   ov2_tracker_describe_brief on the same keyframe (the raw frame is already on the device)
  batch     ov2_describe_brief_batch_d, 4096 images x 308 points, in us per image
and the algorithmic bytes of the batch: per image the union of the 57 x 57 patches of its surviving points, plus 8 B in and 33 B out
per point.  Their share of 8 TB/s needs the kernel time, which comes from a profiler run of its own:
    rocprofv3 --kernel-trace --stats -d <dir> -o brief -- python tools/brief_time.py --batch-only
    python tools/brief_time.py --kernel-stats <dir>
"""
import argparse
import csv
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BPS = 8.0e12


def keyframe_points(w, h, n, rng):
    from ov2slam_amd import synth
    g = synth.grid_keypoints(w, h, 35, rng)
    extra = np.stack([rng.uniform(0, w, n), rng.uniform(0, h, n)], 1)
    return np.concatenate([g, extra])[:n].astype(np.float32)


def patch_union_bytes(pts, w, h):
    """bytes of the union of the 57 x 57 patches [-28, 28]^2 around the surviving points' centres"""
    from tests import brief_ref as R          # the border rule / centres only (tooling, not the product)
    v = R.border_valid(pts, w, h)
    c = R.centres(pts[v]).astype(np.int64)
    m = np.zeros((h + 1, w + 1), np.int32)
    for cx, cy in c:
        m[cy - 28:cy + 29, cx - 28:cx + 29] = 1
    return int(m[:h, :w].sum()), int(v.sum())


def median_us(fn, reps, warm=5):
    for _ in range(warm):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); t.append(time.perf_counter() - t0)
    return float(np.median(t) * 1e6)


def kernel_time_us(path):
    """median k_brief32 duration (us) and call count from rocprofv3's output: its rocpd database (.db) or a kernel_stats.csv
    (--output-format csv; the mean there)"""
    files = [path] if os.path.isfile(path) else glob.glob(os.path.join(path, "**", "*.db"), recursive=True) + \
        glob.glob(os.path.join(path, "**", "*kernel_stats.csv"), recursive=True)
    for f in files:
        if f.endswith(".db"):
            import sqlite3
            d = [r[0] for r in sqlite3.connect(f).execute("select duration from kernels where name like 'k_brief32%'")]
            if d:
                return float(np.median(d)) / 1e3, len(d)
        else:
            for row in csv.DictReader(open(f)):
                if "k_brief32" in row.get("Name", ""):
                    return float(row["AverageNs"]) / 1e3, int(row["Calls"])
    raise SystemExit("no k_brief32 dispatch in %s" % files)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--items", type=int, default=4096)
    ap.add_argument("--points", type=int, default=308)
    ap.add_argument("--batch-only", action="store_true", help="only the batched form (the profiler run)")
    ap.add_argument("--kernel-stats", help="rocprofv3 kernel_stats.csv (or its directory): report the bandwidth share, no GPU work")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    w, h = 752, 480
    rng = np.random.default_rng(0)
    # the batch's points and algorithmic bytes (host arithmetic, seeded: identical in every run)
    bpts = np.stack([keyframe_points(w, h, a.points, np.random.default_rng(100 + b % 64)) for b in range(a.items)])
    ub, nv = zip(*[patch_union_bytes(bpts[b], w, h) for b in range(64)])
    union = float(np.mean(ub)); nvalid = float(np.mean(nv))
    alg_bytes = a.items * (union + a.points * (8 + 33))
    res = dict(w=w, h=h, items=a.items, points=a.points, patch_union_bytes_per_image=union, valid_points_per_image=nvalid,
               algorithmic_bytes=alg_bytes)
    if a.kernel_stats:
        us, calls = kernel_time_us(a.kernel_stats)
        res.update(kernel_us=us, kernel_calls=calls, kernel_us_per_image=us / a.items, achieved_TBps=alg_bytes / (us * 1e-6) / 1e12,
                   share_of_8TBps=alg_bytes / (us * 1e-6) / HBM_BPS)
        print(json.dumps(res))
        return
    import torch
    torch.cuda.init()                  # torch's HIP runtime must be initialised before libov2slam_hip.so in one process
    import ov2slam_amd
    from ov2slam_amd import synth
    ctx = ov2slam_amd.Context(0)
    fx = ov2slam_amd.FeatureExtractor(ctx)
    img = synth.frame_pair(w, h, seed=1)[1]
    pts = keyframe_points(w, h, 616, rng)
    if not a.batch_only:
        res["host_us"] = median_us(lambda: fx.describeBRIEF(img, pts), a.reps)
        vt = ov2slam_amd.VisualFrontEndTracker(ctx, w, h, use_clahe=True)
        vt.trackFrame(img, np.zeros((0, 2), np.float32), np.zeros((0, 2), np.float32), None)
        res["tracker_us"] = median_us(lambda: vt.describeBRIEF(pts), a.reps)
        vt.close()
    tex = synth.base_texture(seed=2)
    base = np.stack([synth.frame_pair(w, h, tex=tex, shift=(5.0 * k, -3.0 * k))[1] for k in range(16)])
    d_img = torch.from_numpy(base).cuda().repeat(a.items // 16 + 1, 1, 1)[:a.items].contiguous()
    d_pts = torch.from_numpy(bpts).cuda()
    d_desc = torch.empty((a.items, a.points, 32), dtype=torch.uint8, device="cuda")
    d_valid = torch.empty((a.items, a.points), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def batch():
        ov2slam_amd.FeatureExtractor.describeBRIEFBatch(ctx, d_img.data_ptr(), w, h, w, w * h, a.items, d_pts.data_ptr(), a.points, 0,
                                                        d_desc.data_ptr(), d_valid.data_ptr())
    reps = 20 if a.batch_only else a.reps
    us = median_us(batch, reps)
    res.update(batch_us=us, batch_us_per_image=us / a.items, host_clock_TBps=alg_bytes / (us * 1e-6) / 1e12)
    ctx.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
