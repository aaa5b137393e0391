"""Randomised parity campaign of detectGFTT (csrc/gftt.hip) against the numpy restatement (tests/gftt_ref.py):

    python tools/fuzz_gftt.py <cases> <seed>

Each case: a random image size 16..400 per side, a row stride != width, content drawn from synthetic frames, noise, constant images
and plateaus of equal dots; a roi mask (random rectangle) or none; 0..n current keypoints (sometimes >= nmaxpts); nbmax -1, small
or large; nmaxdist 0..40; both Sobel dy orders; cornerSubPix on or off.  Prints one JSON line; exit status 1 on any mismatch.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def image(w, h, rng):
    from ov2slam_amd import synth
    k = rng.integers(0, 5)
    if k == 0:
        return rng.integers(0, 256, (h, w)).astype(np.uint8)
    if k == 1:
        return np.full((h, w), int(rng.integers(0, 256)), np.uint8)
    if k == 2:
        img = np.full((h, w), int(rng.integers(0, 200)), np.uint8)
        s = int(rng.integers(3, 12))
        img[s // 2::s, s // 2::s] = 255
        return img
    return synth.frame_pair(w, h, seed=int(rng.integers(0, 1 << 30)))[0]


def main():
    cases, seed = int(sys.argv[1]), int(sys.argv[2])
    import ov2slam_amd
    from ov2slam_amd import _lib as L
    from tests import gftt_ref as R
    rng = np.random.default_rng(seed)
    ctx = ov2slam_amd.Context(0)
    bad, pass2, pts = [], 0, 0
    for c in range(cases):
        w, h = int(rng.integers(16, 401)), int(rng.integers(16, 401))
        img = image(w, h, rng)
        roi = None
        if rng.uniform() < 0.5:
            roi = np.zeros((h, w), np.uint8)
            x0, y0 = int(rng.integers(0, w // 2)), int(rng.integers(0, h // 2))
            roi[y0:y0 + int(rng.integers(1, h)), x0:x0 + int(rng.integers(1, w))] = int(rng.integers(1, 256))
        nmaxpts = int(rng.integers(1, 500))
        nmaxdist = int(rng.integers(0, 41))
        q = float(10 ** rng.uniform(-4, -0.5))
        ncur = int(rng.integers(0, nmaxpts + 20)) if rng.uniform() < 0.3 else int(rng.integers(0, 30))
        cur = np.stack([rng.uniform(-5, w + 5, ncur), rng.uniform(-5, h + 5, ncur)], 1).astype(np.float32)
        nbmax = [-1, int(rng.integers(1, 20)), int(rng.integers(1, 600))][int(rng.integers(0, 3))]
        sub, dy = bool(rng.integers(0, 2)), int(rng.integers(0, 2))
        fx = ov2slam_amd.FeatureExtractor(ctx, dmaxquality=q, nmaxpts=nmaxpts, nmaxdist=nmaxdist)
        buf = np.full((h, w + 5), 1, np.uint8); buf[:, :w] = img
        ctx.set_option(L.OV2_OPT_SOBEL_DY_ORDER, dy)
        got = fx.detectGFTT(buf[:, :w], cur, roi, nbmax=nbmax, subpix=sub)
        info = {}
        ref = R.detect_gftt(img, cur, roi, nbmax, R.params(nmaxpts, nmaxdist, q), subpix=sub, dy_order=dy, info=info)
        pass2 += bool(info.get("pass2"))
        pts += len(ref)
        if got.shape != ref.shape or not np.array_equal(got.view(np.uint32), ref.view(np.uint32)):
            bad.append(dict(case=c, w=w, h=h, n_gpu=len(got), n_ref=len(ref)))
    ctx.set_option(L.OV2_OPT_SOBEL_DY_ORDER, 0)
    ctx.close()
    print(json.dumps(dict(cases=cases, seed=seed, mismatches=len(bad), pass2_cases=pass2, points=pts, first=bad[:5])))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
