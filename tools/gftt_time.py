"""Wall time of detectGFTT on the GPU (csrc/gftt.hip), host synchronisation included:

    python tools/gftt_time.py [reps]

Prints one JSON line: us per keyframe of the host-image form and of the pyramid (_d) form on a synthetic EuRoC frame (752x480,
5-px roi, 308 points, minDistance 35 -- the pass-2 branch runs) and us per image of the batched form at 4096 items (376x240 and
752x480), next to detectSingleScale's pyramid form on the same frame.
"""
import json
import os
import sys
import time

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
    import torch
    torch.cuda.init()
    import ov2slam_amd
    from ov2slam_amd import synth
    ctx = ov2slam_amd.Context(0)
    w, h = 752, 480
    img = synth.frame_pair(w, h, seed=1234)[0]
    roi = np.zeros((h, w), np.uint8); roi[5:h - 5, 5:w - 5] = 255
    fx = ov2slam_amd.FeatureExtractor(ctx, dmaxquality=0.001, nmaxpts=308, nmaxdist=35)
    P = ov2slam_amd.Pyramid(ctx, w, h, 9, 3).build(img)
    none = np.zeros((0, 2), np.float32)
    r = dict(host_us=best(lambda: fx.detectGFTT(img, none, roi), reps),
             pyr_us=best(lambda: fx.detectGFTTPyr(P, none, roi), reps),
             singlescale_pyr_us=best(lambda: fx.detectSingleScalePyr(P, 35, none, (5, 5, w - 10, h - 10)), reps),
             npts=int(len(fx.detectGFTTPyr(P, none, roi))))
    for bw, bh in ((376, 240), (752, 480)):
        B = 4096
        base = [synth.frame_pair(bw, bh, seed=k)[0] for k in range(8)]
        PB = ov2slam_amd.Pyramid(ctx, bw, bh, 9, 0, batch=B).build(np.stack([base[b % 8] for b in range(B)]))
        ctx.sync()
        d_out = torch.zeros((B, 308, 2), dtype=torch.float32, device="cuda")
        nb = np.full(B, -1, np.int32)
        p = fx.gftt_params()
        t = best(lambda: ov2slam_amd.FeatureExtractor.detectGFTTBatch(ctx, PB, 0, 0, p, 0, 0, 0, nb, d_out.data_ptr(), 308), 2)
        r["batch4096_%dx%d_us_per_image" % (bw, bh)] = t / B
        del PB
    ctx.close()
    print(json.dumps(r))


if __name__ == "__main__":
    main()
