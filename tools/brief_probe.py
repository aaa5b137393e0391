"""Inputs for pinning describeBRIEF against a real OpenCV build (tools/ref_capture/capture_brief.cpp runs OpenCV on them).

Two kinds of input set, each written as <name>.img (n images x h x w bytes), <name>.kp (k x 2 float32: the same k keypoints are
described on every image of a set) and one line "name n w h k" in sets.txt:
  probe_bright / probe_dark   57 x 57 images, one keypoint at (28, 28), one pixel q set (255 on black / 0 on white), for each of
                              the 3249 positions of q.  Bit t of the bright probe at q is set iff q lies in box(b) \\ box(a), of the
                              dark one iff q lies in box(a) \\ box(b): together they determine OpenCV's 256 test pairs
                              (tools/brief_pattern_from_probes.py).
  euroc / kitti               synthetic 752 x 480 / 1241 x 376 frames (seeded) with fractional keypoints: a jittered grid, random
                              points, the border bands [27, 29] and [W-30, W-27], exact .5 coordinates including W-28.5 / H-28.5
The whole procedure (needs OpenCV with contrib; not in this repository's build image):
    python tools/brief_probe.py /tmp/brief_in
    cmake -S tools/ref_capture -B /tmp/ref_capture && cmake --build /tmp/ref_capture --target ov2_capture_brief
    mkdir -p /tmp/brief_out && /tmp/ref_capture/ov2_capture_brief /tmp/brief_in /tmp/brief_out
    python tools/brief_pattern_from_probes.py /tmp/brief_out      # -> tests/golden/brief_pattern_opencv.npy, tests/golden/brief_opencv/
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PROBE = 57
FRAME_SETS = (("euroc", 752, 480, 11), ("kitti", 1241, 376, 12))


def probe_images():
    """-> (bright, dark): (3249, 57, 57) uint8 each; image k has pixel (k // 57, k % 57) set"""
    n = PROBE * PROBE
    bright = np.zeros((n, PROBE, PROBE), np.uint8)
    dark = np.full((n, PROBE, PROBE), 255, np.uint8)
    k = np.arange(n)
    bright[k, k // PROBE, k % PROBE] = 255
    dark[k, k // PROBE, k % PROBE] = 0
    return bright, dark


def probe_keypoints():
    return np.array([[28.0, 28.0]], np.float32)


def frame_keypoints(w, h, rng):
    """a jittered grid, random points, the border bands and exact .5 coordinates (the odd-size corner case included)"""
    from ov2slam_amd import synth
    grid = synth.grid_keypoints(w, h, 35, rng)
    rnd = np.stack([rng.uniform(0, w, 200), rng.uniform(0, h, 200)], 1)
    band = []
    for v in np.arange(27.0, 29.01, 0.25):
        band += [(v, h / 2), (w / 2, v), (w - 57.0 + v, h / 3), (w / 3, h - 57.0 + v)]     # [27, 29] and [W-30, W-28]
    for v in np.arange(w - 30.0, w - 26.99, 0.25):
        band.append((v, h / 2 + 3))
    for v in np.arange(h - 30.0, h - 26.99, 0.25):
        band.append((w / 2 + 3, v))
    half = [(27.5, 100.5), (28.5, 101.5), (w - 28.5, h / 2 + 0.5), (w / 2 + 0.5, h - 28.5), (w - 28.5, h - 28.5),
            (w - 29.5, 60.5), (80.5, h - 29.5), (100.5, 200.5), (101.5, 201.5)]
    return np.concatenate([grid, rnd, np.array(band), np.array(half)]).astype(np.float32)


def frame_sets():
    """-> list of (name, images (n, h, w) uint8, keypoints (k, 2) float32), seeded"""
    from ov2slam_amd import synth
    out = []
    for name, w, h, seed in FRAME_SETS:
        prev, cur, _ = synth.frame_pair(w, h, seed=seed)
        rng = np.random.default_rng(seed)
        out.append((name, np.stack([prev, cur]).astype(np.uint8), frame_keypoints(w, h, rng)))
    return out


def all_sets():
    bright, dark = probe_images()
    kp = probe_keypoints()
    return [("probe_bright", bright, kp), ("probe_dark", dark, kp)] + frame_sets()


def write(outdir):
    os.makedirs(outdir, exist_ok=True)
    with open(os.path.join(outdir, "sets.txt"), "w") as man:
        for name, imgs, kps in all_sets():
            n, h, w = imgs.shape
            np.ascontiguousarray(imgs, np.uint8).tofile(os.path.join(outdir, name + ".img"))
            np.ascontiguousarray(kps, np.float32).tofile(os.path.join(outdir, name + ".kp"))
            man.write("%s %d %d %d %d\n" % (name, n, w, h, len(kps)))
    print("wrote %s" % outdir)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit("usage: brief_probe.py <outdir>")
    write(sys.argv[1])
