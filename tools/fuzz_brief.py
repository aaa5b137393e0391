"""Randomised parity campaign of describeBRIEF (csrc/brief.hip) against the numpy restatement (tests/brief_ref.py):

    python tools/fuzz_brief.py <cases> <seed>

Each case: a random image size 57..1300 per side (odd and even), a row stride != width, random or constant content, the built-in or
a random pattern, keypoints that mix random floats, the border bands, exact .5 coordinates (the odd-size corner case included),
duplicates, negatives and non-finite values.  Every fourth case also runs the batched form (ov2_describe_brief_batch_d) on a few
items of that size with per-item counts from 0 to the capacity.  Prints one JSON line; exit status 1 on any mismatch.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def points(w, h, rng):
    n = int(rng.integers(1, 400))
    p = [np.stack([rng.uniform(-20, w + 20, n), rng.uniform(-20, h + 20, n)], 1)]
    k = int(rng.integers(0, 40))
    edge = np.stack([rng.choice([27.0, 27.5, 28.0, 28.5, 29.0, w - 30.0, w - 29.5, w - 29.0, w - 28.5, w - 28.0, w - 27.0], k),
                     rng.choice([27.0, 27.5, 28.0, 28.5, 29.0, h - 30.0, h - 29.5, h - 29.0, h - 28.5, h - 28.0, h - 27.0], k)], 1)
    p.append(edge)
    p.append(np.floor(p[0][:k]) + 0.5)
    p.append(np.array([[np.nan, 40.0], [40.0, np.inf], [-1e9, 5.0]])[:int(rng.integers(0, 4))].reshape(-1, 2))
    out = np.concatenate(p).astype(np.float32)
    if len(out) and rng.uniform() < 0.5:
        out = np.concatenate([out, out[rng.integers(0, len(out), 8)]])
    return out[rng.permutation(len(out))]


def main():
    cases, seed = int(sys.argv[1]), int(sys.argv[2])
    import torch
    torch.cuda.init()                  # torch's HIP runtime must be initialised before libov2slam_hip.so in one process
    import ov2slam_amd
    from tests import brief_ref as R
    rng = np.random.default_rng(seed)
    ctx = ov2slam_amd.Context(0)
    fx = ov2slam_amd.FeatureExtractor(ctx)
    builtin = ctx.brief_pattern()
    bad, npts, nbatch = [], 0, 0
    for c in range(cases):
        w, h = (int(v) for v in rng.integers(57, 1301, 2))
        if rng.uniform() < 0.1:
            w = int(rng.integers(57, 64))
        img = rng.integers(0, 256, (h, w), dtype=np.uint8) if rng.uniform() < 0.8 else np.full((h, w), int(rng.integers(0, 256)), np.uint8)
        pat = builtin if rng.uniform() < 0.3 else rng.integers(-24, 25, (256, 4)).astype(np.int8)
        ctx.set_brief_pattern(pat)
        pad = int(rng.integers(1, 70))
        buf = np.zeros((h, w + pad), np.uint8); buf[:, :w] = img
        pts = points(w, h, rng)
        npts += len(pts)
        d, v = fx.describeBRIEF(buf[:, :w], pts)
        rd, rv = R.describe(img, pts, pat)
        if not (np.array_equal(d, rd) and np.array_equal(v, rv)):
            bad.append(dict(case=c, form="host", w=w, h=h, n=len(pts)))
        if c % 4 == 3:
            B = int(rng.integers(1, 6))
            cap = int(rng.integers(1, 200))
            imgs = rng.integers(0, 256, (B, h, w), dtype=np.uint8)
            P = np.stack([np.resize(points(w, h, rng), (cap, 2)) for _ in range(B)]).astype(np.float32)
            nn = rng.integers(0, cap + 1, B).astype(np.int32)
            pitch = w + pad
            stride = pitch * h + int(rng.integers(0, 300))
            flat = np.zeros((B, stride), np.uint8)
            for b in range(B):
                flat[b, :pitch * h].reshape(h, pitch)[:, :w] = imgs[b]
            t_img = torch.from_numpy(flat).cuda(); t_p = torch.from_numpy(P).cuda(); t_n = torch.from_numpy(nn).cuda()
            t_d = torch.zeros((B, cap, 32), dtype=torch.uint8, device="cuda"); t_v = torch.zeros((B, cap), dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            fx.describeBRIEFBatch(ctx, t_img.data_ptr(), w, h, pitch, stride, B, t_p.data_ptr(), cap, t_n.data_ptr(), t_d.data_ptr(), t_v.data_ptr())
            gd, gv = t_d.cpu().numpy(), t_v.cpu().numpy().astype(bool)
            nbatch += 1
            for b in range(B):
                k = int(nn[b])
                rd, rv = R.describe(imgs[b], P[b, :k], pat)
                if not (np.array_equal(gd[b, :k], rd) and np.array_equal(gv[b, :k], rv) and not gd[b, k:].any()):
                    bad.append(dict(case=c, form="batch", item=b, w=w, h=h, n=k))
    ctx.set_brief_pattern(None)
    ctx.close()
    print(json.dumps(dict(cases=cases, seed=seed, points=npts, batch_calls=nbatch, mismatches=len(bad), first=bad[:5])))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
