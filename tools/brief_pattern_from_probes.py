"""Recovers OpenCV's 256 BRIEF test pairs from the descriptors capture_brief.cpp dumped for the probe images of
tools/brief_probe.py, and files the OpenCV-side results under tests/golden/:

    python tools/brief_pattern_from_probes.py <capture dir>
        -> tests/golden/brief_pattern_opencv.npy    (256, 4) int8 rows {ay, ax, by, bx}, for Context.set_brief_pattern
        -> tests/golden/brief_opencv/<set>.desc.npy / <set>.valid.npy for the euroc / kitti frame sets

With a single pixel q set in a 57 x 57 image described at (28, 28), the 9x9 sums are 255 * [q in box] (bright on black) or
81 * 255 - 255 * [q in box] (dark on white).  So bit t of the bright probe at q is set iff q is in box(b) \\ box(a), of the dark probe
iff q is in box(a) \\ box(b).  A 9x9 box is found from its difference with another one: where the two boxes differ in rows, the
difference spans all 9 columns of the box (and the other way round); where one extent is cut short, it is cut on the side of the
other box.  A pair with a == b never sets its bit: it is recorded as (0, 0, 0, 0).  Every recovered pair is checked by rebuilding
both difference sets.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 57
C = 28          # the probe keypoint's centre


def _box(cy, cx):
    m = np.zeros((P, P), bool)
    m[C + cy - 4:C + cy + 5, C + cx - 4:C + cx + 5] = True
    return m


def _centre(own, other):
    """centre offset (dy, dx) of the box whose difference with the other box is `own` (both difference sets non-empty)"""
    out = []
    for axis in (0, 1):
        lines = np.nonzero(own.any(axis=1 - axis))[0]
        other_lines = np.nonzero(other.any(axis=1 - axis))[0]
        lo, hi = lines.min(), lines.max()
        if hi - lo == 8 or other_lines.min() > lo:
            out.append(lo + 4 - C)                 # the full extent, or cut short at the far side
        else:
            out.append(hi - 4 - C)
    return out


def recover(bright_desc, dark_desc):
    """bright_desc / dark_desc: (3249, 32) uint8, row k = the probe with pixel (k // 57, k % 57) -> (256, 4) int8"""
    bb = np.unpackbits(np.asarray(bright_desc, np.uint8).reshape(P * P, 32), axis=1, bitorder="big").astype(bool)
    db = np.unpackbits(np.asarray(dark_desc, np.uint8).reshape(P * P, 32), axis=1, bitorder="big").astype(bool)
    pairs = np.zeros((256, 4), np.int8)
    for t in range(256):
        b_minus_a = bb[:, t].reshape(P, P)
        a_minus_b = db[:, t].reshape(P, P)
        if not a_minus_b.any() and not b_minus_a.any():
            continue                                # a == b: the test is constant 0
        if not a_minus_b.any() or not b_minus_a.any():
            raise ValueError("test %d: only one of the two difference sets is non-empty -- not two 9x9 boxes" % t)
        ay, ax = _centre(a_minus_b, b_minus_a)
        by, bx = _centre(b_minus_a, a_minus_b)
        A, B = _box(ay, ax), _box(by, bx)
        if not (np.array_equal(A & ~B, a_minus_b) and np.array_equal(B & ~A, b_minus_a)):
            raise ValueError("test %d: the probe bits are not explained by one pair of 9x9 boxes" % t)
        pairs[t] = (ay, ax, by, bx)
    return pairs


def main(capdir):
    def load(name):
        return np.load(os.path.join(capdir, name + ".desc.npy")), np.load(os.path.join(capdir, name + ".valid.npy"))
    bd, bv = load("probe_bright")
    dd, dv = load("probe_dark")
    if not (bv.all() and dv.all()):
        raise SystemExit("the probe keypoint (28, 28) was rejected in some probe image: not the border rule this assumes")
    pairs = recover(bd.reshape(P * P, 32), dd.reshape(P * P, 32))
    gold = os.path.join(ROOT, "tests", "golden")
    np.save(os.path.join(gold, "brief_pattern_opencv.npy"), pairs)
    os.makedirs(os.path.join(gold, "brief_opencv"), exist_ok=True)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import brief_probe
    for name, _, _, _ in brief_probe.FRAME_SETS:
        d, v = load(name)
        np.save(os.path.join(gold, "brief_opencv", name + ".desc.npy"), d)
        np.save(os.path.join(gold, "brief_opencv", name + ".valid.npy"), v)
    print("recovered %d non-degenerate pairs -> %s" % (int((pairs != 0).any(axis=1).sum()), os.path.join(gold, "brief_pattern_opencv.npy")))


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit("usage: brief_pattern_from_probes.py <capture dir>")
    main(sys.argv[1])
