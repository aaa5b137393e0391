"""Numpy specification of the loop closer's keyframe preparation (the reference's LoopCloser::run, src/loop_closer.cpp:86-144: the
exclusion mask, FastFeatureDetector(20) on the whole raw image, KeyPointsFilter::retainBest(300), BriefDescriptorExtractor::compute),
written twice, as tests/knn_ref.py is:

  replay(img, excl, ...)  transcribes the path the reference takes, step by step: cv::FAST with non-maximum suppression (the
      oracle's orc_fast9_16), a byte mask that is 255 everywhere with cv::circle(mask, px, radius, 0, -1) painted by the oracle's
      orc_circle_fill0 at the np.rint centres, KeyPointsFilter::runByPixelsMask (the mask byte at the corner), retainBest through a
      SORT of the responses (the retain-th largest is the boundary, everything >= it stays), runByImageBorder(28), and
      tests/brief_ref.py for the descriptor bytes.
  flat(img, excl, ...)    states the same order-free and without the oracle: the corner test and the score as maxima over the
      sixteen 9-pixel arcs (cornerScore<16> of a corner is the largest threshold at which the pixel would still be one: the best
      arc's least extreme difference, minus one), the suppression on the score map, the exclusion as a distance table (|dy| <= radius and
      |dx| <= halfwidth[|dy|] of the midpoint circle), and the cut from a 256-bin histogram.  This is the form the GPU tests
      compare against.

Both return a dict: n_all, cut, n_kept, n_desc (ints); all_xy (n_all, 2) int16, all_resp (n_all,) uint8: the corners after the
mask filter; kept_xy, kept_resp: the retained ones; kept_valid (n_kept,) uint8: inside the BRIEF border; kept_desc (n_kept, 32)
uint8 (zero rows where kept_valid is 0).  Every list is in raster order (y, then x).  cut is the retain-th largest response, 0
when nothing was cut (retain < 0, retain == 0, or at most `retain` corners).

cv::FAST, KeyPointsFilter and BriefDescriptorExtractor::compute are restated from OpenCV's published source, not pinned against an
OpenCV build: there is none here.

Kept as defined:
  * the suppression is strict: two equal neighbouring scores remove each other;
  * a neighbour outside the candidate range 3 <= x < w-3, 3 <= y < h-3 counts as 0; an image with w < 7 or h < 7 has no corners;
  * with threshold 0 a corner can score 0; it never survives the suppression, so responses are 1 .. 255;
  * the exclusion centre is (rint(px), rint(py)), half to even; a point with a non-finite coordinate paints nothing;
  * ties at the cut are all kept, so n_kept > retain is normal; the border filter comes after retainBest."""
import os
import re

import numpy as np

from tests import brief_ref

THRESHOLD, RETAIN, RADIUS = 20, 300, 2
BORDER = brief_ref.BORDER
FIELDS = ("n_all", "cut", "n_kept", "n_desc", "all_xy", "all_resp", "kept_xy", "kept_resp", "kept_valid", "kept_desc")
# the circle of radius 3 in cv::FAST's order (dx, dy)
RING = [(0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3), (0, -3), (-1, -3), (-2, -2), (-3, -1), (-3, 0), (-3, 1), (-2, 2), (-1, 3)]


def builtin_pattern():
    """the BRIEF test pairs a context starts with (ov2slam_amd/csrc/brief_pattern.hpp)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    txt = open(os.path.join(root, "ov2slam_amd", "csrc", "brief_pattern.hpp")).read()
    body = txt[txt.index("= {") + 3:txt.index("};")]
    return np.array([int(v) for v in re.findall(r"-?\d+", body)], np.int8).reshape(256, 4)


def _excl(excl):
    e = np.zeros((0, 2), np.float32) if excl is None else np.asarray(excl, np.float32)
    return e.reshape(-1, 2)


def centres(excl):
    """(rint(px), rint(py)) of the points that paint at all, as int64 (n, 2)"""
    e = _excl(excl)
    ok = np.isfinite(e).all(axis=1)
    with np.errstate(invalid="ignore"):
        c = np.clip(np.rint(e[ok].astype(np.float64)), -2.0 ** 40, 2.0 ** 40)     # (far outside any image either way)
    return c.astype(np.int64)


def halfwidths(radius):
    """the midpoint circle of drawing.cpp Circle() as half-widths: row +-k of a filled circle spans cx - hw[k] .. cx + hw[k]; -1: none"""
    hw = [-1] * (radius + 1)
    err, dx, dy, plus, minus = 0, radius, 0, 1, (radius << 1) - 1
    while dx >= dy:
        hw[dy] = max(hw[dy], dx)
        hw[dx] = max(hw[dx], dy)
        dy += 1
        err += plus
        plus += 2
        m = (1 if err <= 0 else 0) - 1
        err -= minus & m
        dx += m
        minus -= m & 2
    return np.array(hw, np.int64)


def _pack(img, xs, ys, resp, keep, cut, pattern):
    """the result dict from the masked corners in raster order and the retained flags"""
    h, w = img.shape
    all_xy = np.stack([xs, ys], axis=1).astype(np.int16).reshape(-1, 2)
    all_resp = np.asarray(resp, np.uint8)
    kept_xy, kept_resp = all_xy[keep], all_resp[keep]
    desc, valid = brief_ref.describe(img, kept_xy.astype(np.float32), pattern)
    return dict(n_all=int(len(all_xy)), cut=int(cut), n_kept=int(len(kept_xy)), n_desc=int(valid.sum()), all_xy=all_xy, all_resp=all_resp,
                kept_xy=kept_xy, kept_resp=kept_resp, kept_valid=valid.astype(np.uint8), kept_desc=desc)


def replay(img, excl, pattern, threshold=THRESHOLD, retain=RETAIN, radius=RADIUS):
    from oracle import oracle as O
    img = np.ascontiguousarray(img, np.uint8)
    h, w = img.shape
    xs, ys, sc = O.fast9_16(img, threshold, True)                       # raster order
    mask = np.full((h, w), 255, np.uint8)
    for cx, cy in centres(excl):
        if abs(cx) < 2 ** 30 and abs(cy) < 2 ** 30:                     # (the C int of the painter)
            mask = O.circle_fill0(mask, int(cx), int(cy), radius)
    ok = mask[ys, xs] != 0                                              # runByPixelsMask
    xs, ys, sc = xs[ok], ys[ok], sc[ok]
    keep = np.ones(len(sc), bool)
    cut = 0
    if retain >= 0 and len(sc) > retain:                                # retainBest
        if retain == 0:
            keep[:] = False
        else:
            cut = int(np.sort(sc)[::-1][retain - 1])
            keep = sc >= cut
    return _pack(img, xs, ys, sc, keep, cut, pattern)


def score_map(img, threshold):
    """(h, w) int32: cornerScore<16> of every FAST-9/16 corner in the candidate range, -1 where the pixel is no corner"""
    img = np.ascontiguousarray(img, np.uint8).astype(np.int32)
    h, w = img.shape
    out = np.full((h, w), -1, np.int32)
    if w < 7 or h < 7:
        return out
    t = min(max(int(threshold), 0), 255)
    v = img[3:h - 3, 3:w - 3]
    d = np.stack([v - img[3 + dy:h - 3 + dy, 3 + dx:w - 3 + dx] for dx, dy in RING])       # centre minus ring pixel
    d2 = np.concatenate([d, d[:8]])
    # per arc of 9 contiguous ring pixels: how dark / how bright its least extreme pixel is
    dark = np.max(np.stack([d2[s:s + 9].min(axis=0) for s in range(16)]), axis=0)
    bright = np.max(np.stack([(-d2[s:s + 9]).min(axis=0) for s in range(16)]), axis=0)
    best = np.maximum(dark, bright)
    out[3:h - 3, 3:w - 3] = np.where(best > t, best - 1, -1)
    return out


def corners(img, threshold):
    """the corners that survive the strict 3x3 suppression, raster order -> (xs, ys, scores)"""
    s = np.maximum(score_map(img, threshold), 0)                        # not a corner: 0
    h, w = s.shape
    p = np.zeros((h + 2, w + 2), np.int32)
    p[1:-1, 1:-1] = s
    best = np.max(np.stack([p[1 + dy:h + 1 + dy, 1 + dx:w + 1 + dx] for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dx, dy) != (0, 0)]), axis=0)
    ys, xs = np.nonzero(s > best)
    return xs, ys, s[ys, xs]


def excluded(xs, ys, excl, radius, w, h):
    """per corner: does some exclusion point's filled circle cover it (the corners lie inside the image, so clipping changes nothing)"""
    c = centres(excl)
    out = np.zeros(len(xs), bool)
    if len(c) == 0 or len(xs) == 0:
        return out
    hw = halfwidths(radius)
    for i in range(0, len(xs), 4096):
        dx = np.abs(xs[i:i + 4096, None].astype(np.int64) - c[None, :, 0])
        dy = np.abs(ys[i:i + 4096, None].astype(np.int64) - c[None, :, 1])
        inrow = dy <= radius
        half = hw[np.where(inrow, dy, 0)]
        out[i:i + 4096] = (inrow & (dx <= half)).any(axis=1)
    return out


def cut_of(resp, retain):
    """(cut, smallest retained response) from the 256-bin histogram; the second is 256 when nothing is retained"""
    hist = np.bincount(np.asarray(resp, np.int64), minlength=256)
    if retain == 0:
        return 0, 256
    if retain < 0 or hist.sum() <= retain:
        return 0, 1
    above = np.cumsum(hist[::-1])[::-1]                                 # above[v]: responses >= v
    c = int(np.nonzero(above >= retain)[0].max())
    return c, c


def flat(img, excl, pattern, threshold=THRESHOLD, retain=RETAIN, radius=RADIUS):
    img = np.ascontiguousarray(img, np.uint8)
    h, w = img.shape
    xs, ys, sc = corners(img, threshold)
    ok = ~excluded(xs, ys, excl, radius, w, h)
    xs, ys, sc = xs[ok], ys[ok], sc[ok]
    cut, lowest = cut_of(sc, retain)
    return _pack(img, xs, ys, sc, sc >= lowest, cut, pattern)


def same(a, b):
    """(True, None) or (False, the first field that differs)"""
    for f in FIELDS:
        x, y = np.asarray(a[f]), np.asarray(b[f])
        if x.shape != y.shape or x.dtype != y.dtype or x.tobytes() != y.tobytes():
            return False, f
    return True, None


def kept_indices(all_resp, retain):
    """indices into the masked corner list of the set retainBest keeps (whatever order the reference leaves it in)"""
    _, lowest = cut_of(all_resp, retain)
    return np.nonzero(np.asarray(all_resp, np.int64) >= lowest)[0]


# ---- cases ---------------------------------------------------------------------------------------------------------------------
def dots(w, h, pts, bg=0):
    """an image that is `bg` everywhere with single pixels (x, y, value): an isolated pixel brighter than the background by more
    than the threshold is a corner of score value - bg - 1, and nothing around it is"""
    img = np.full((h, w), bg, np.uint8)
    for x, y, v in pts:
        img[y, x] = v
    return img


def textured(rng, w, h):
    """blocks, blobs and noise: thousands of corners per 100k pixels with many equal scores"""
    img = rng.integers(90, 110, (h, w)).astype(np.int32)
    for _ in range(max(4, w * h // 400)):
        x, y = int(rng.integers(0, w)), int(rng.integers(0, h))
        bw, bh = int(rng.integers(1, 12)), int(rng.integers(1, 12))
        img[y:y + bh, x:x + bw] = int(rng.integers(0, 256))
    return np.clip(img, 0, 255).astype(np.uint8)


def make_case(rng, w, h, n_excl, kind="textured", threshold=THRESHOLD):
    """(img, excl): excl has n_excl points -- a third on or next to corners of the image (so that circles remove some and just miss
    others), some at x.5 / y.5, some outside the image or on its edges, the rest anywhere"""
    if kind == "noise":
        img = rng.integers(0, 256, (h, w), dtype=np.uint8)
    elif kind == "flat":
        img = np.full((h, w), int(rng.integers(0, 256)), np.uint8)
    else:
        img = textured(rng, w, h)
    xs, ys, _ = corners(img, threshold)
    e = np.zeros((n_excl, 2), np.float32)
    for i in range(n_excl):
        r = i % 6
        if r < 2 and len(xs):
            j = int(rng.integers(0, len(xs)))
            e[i] = (xs[j] + int(rng.integers(-3, 4)), ys[j] + int(rng.integers(-3, 4)))
        elif r == 2:
            e[i] = (int(rng.integers(0, w)) + 0.5, int(rng.integers(0, h)) + 0.5)
        elif r == 3:
            e[i] = [(-1.0, float(rng.integers(0, h))), (float(w), float(rng.integers(0, h))), (float(rng.integers(0, w)), -2.0),
                    (float(rng.integers(0, w)), h + 1.0), (0.0, 0.0), (w - 1.0, h - 1.0)][int(rng.integers(0, 6))]
        else:
            e[i] = (rng.uniform(-3, w + 3), rng.uniform(-3, h + 3))
    return img, e


def crafted_cases(tile_w, tile_h):
    """(name, img, excl, params dict, expected dict of literals: n_all, cut, n_kept, n_desc, kept (list of (x, y, resp)))"""
    T, U = tile_w, tile_h
    P = dict(threshold=20, retain=300, radius=2)
    cases = []
    # two equal neighbours remove each other; of two unequal neighbours the larger stays; (30, 10) is alone
    img = dots(60, 40, [(10, 10, 200), (11, 10, 200), (20, 10, 200), (21, 11, 150), (30, 10, 100)])
    cases.append(("nms_tie", img, None, P, dict(n_all=2, cut=0, n_kept=2, n_desc=0, kept=[(20, 10, 199), (30, 10, 99)])))
    # the candidate range: columns 3 and w-4, rows 3 and h-4 are in, columns 2 and w-3, rows 2 and h-3 are out
    img = dots(50, 40, [(3, 10, 200), (46, 10, 200), (20, 3, 200), (20, 36, 200), (2, 20, 200), (47, 20, 200), (30, 2, 200), (30, 37, 200)])
    cases.append(("candidate_range", img, None, P, dict(n_all=4, cut=0, n_kept=4, n_desc=0,
                                                        kept=[(20, 3, 199), (3, 10, 199), (46, 10, 199), (20, 36, 199)])))
    # the same across the kernel's tiles: pairs that straddle a tile edge in x and in y, a corner in each of four tiles' corners
    w, h = 2 * T + 9, 2 * U + 9
    img = dots(w, h, [(T - 1, 5, 200), (T, 5, 200), (T - 1, 9, 200), (T, 9, 150), (7, U - 1, 150), (7, U, 200), (20, U - 1, 90), (21, U, 90),
                      (T + 3, U + 3, 60), (2 * T, 2 * U, 70), (2 * T + 5, 2 * U + 5, 80)])
    cases.append(("tile_edges", img, None, P, dict(n_all=5, cut=0, n_kept=5, n_desc=0,
                                                   kept=[(T - 1, 9, 199), (7, U, 199), (T + 3, U + 3, 59), (2 * T, 2 * U, 69), (2 * T + 5, 2 * U + 5, 79)])))
    # radius 0 paints the one pixel (rint(x), rint(y)): 10.5 -> 10, 11.5 -> 12, 20.5 -> 20 in y, 21.5 -> 22
    img = dots(60, 70, [(10, 20, 200), (11, 30, 200), (12, 40, 200), (11, 50, 200), (40, 20, 200), (40, 31, 200), (40, 42, 200), (40, 51, 200)])
    excl = [(10.5, 20), (10.5, 30), (11.5, 40), (11.5, 50), (40, 20.5), (40, 30.5), (40, 41.5), (40, 51.5)]
    cases.append(("half_to_even", img, excl, dict(P, radius=0), dict(n_all=4, cut=0, n_kept=4, n_desc=0,
                                                                     kept=[(11, 30, 199), (40, 31, 199), (11, 50, 199), (40, 51, 199)])))
    # radius 2 is row 0 with half-width 2, rows +-1 with 1 and rows +-2 with 0: the outermost pixels remove, one step further keeps
    img = dots(80, 60, [(12, 10, 200), (33, 10, 200), (50, 12, 200), (71, 12, 200), (11, 31, 200), (32, 31, 200), (50, 43, 200)])
    excl = [(10, 10), (30, 10), (50, 10), (70, 10), (10, 30), (30, 30), (50, 40), (float("nan"), 10), (12, float("inf")), (-np.inf, np.nan)]
    cases.append(("circle_edge", img, excl, P, dict(n_all=4, cut=0, n_kept=4, n_desc=1,
                                                    kept=[(33, 10, 199), (71, 12, 199), (32, 31, 199), (50, 43, 199)])))
    # circles clipped by each edge of the image (centres at distance 1 inside) and centred outside it (radius 4 reaches column 3)
    img = dots(40, 40, [(3, 10, 200), (36, 10, 200), (10, 3, 200), (10, 36, 200), (3, 25, 200), (36, 25, 200), (25, 3, 200), (25, 36, 200)])
    excl = [(1, 10), (38, 10), (10, 1), (10, 38)]
    cases.append(("clipped", img, excl, P, dict(n_all=4, cut=0, n_kept=4, n_desc=0, kept=[(25, 3, 199), (3, 25, 199), (36, 25, 199), (25, 36, 199)])))
    excl = [(-1, 10), (40, 10), (10, -1), (10, 40), (-5, 25), (44, 25), (25, -6), (25, 1e30)]
    cases.append(("centred_outside", img, excl, dict(P, radius=4), dict(n_all=4, cut=0, n_kept=4, n_desc=0,
                                                                         kept=[(25, 3, 199), (3, 25, 199), (36, 25, 199), (25, 36, 199)])))
    # retainBest
    five = [(30, 30, 200), (40, 30, 150), (50, 30, 121), (60, 30, 121), (70, 30, 100)]
    img = dots(100, 100, five)
    k = lambda idx: [(five[i][0], five[i][1], five[i][2] - 1) for i in idx]
    cases.append(("fewer_than_retain", img, None, dict(P, retain=5), dict(n_all=5, cut=0, n_kept=5, n_desc=5, kept=k(range(5)))))
    cases.append(("retain_plus_one_tie", dots(100, 100, five[:4]), None, dict(P, retain=3), dict(n_all=4, cut=120, n_kept=4, n_desc=4, kept=k(range(4)))))
    cases.append(("cut_without_tie", img, None, dict(P, retain=2), dict(n_all=5, cut=149, n_kept=2, n_desc=2, kept=k(range(2)))))
    cases.append(("tie_at_cut", img, None, dict(P, retain=3), dict(n_all=5, cut=120, n_kept=4, n_desc=4, kept=k(range(4)))))
    cases.append(("retain_zero", img, None, dict(P, retain=0), dict(n_all=5, cut=0, n_kept=0, n_desc=0, kept=[])))
    cases.append(("retain_all", img, None, dict(P, retain=-1), dict(n_all=5, cut=0, n_kept=5, n_desc=5, kept=k(range(5)))))
    eq = [(10 + 9 * i, 10 + 8 * j, 180) for j in range(4) for i in range(5)]
    cases.append(("all_equal", dots(70, 50, eq), None, dict(P, retain=3), dict(n_all=20, cut=179, n_kept=20, n_desc=0,
                                                                                 kept=[(x, y, 179) for x, y, _ in eq])))
    # the border filter comes after retainBest: the two best corners lie outside [28, w-28) x [28, h-28)
    img = dots(100, 100, [(27, 50, 250), (72, 50, 240), (28, 28, 100), (71, 71, 90), (50, 50, 80)])
    cases.append(("border_after_retain", img, None, dict(P, retain=3), dict(n_all=5, cut=99, n_kept=3, n_desc=1,
                                                                             kept=[(28, 28, 99), (27, 50, 249), (72, 50, 239)])))
    # threshold: clamped to [0, 255]; a dot of 21 over 0 passes threshold 20, one of 20 does not; dark dots on a bright background
    img = dots(60, 40, [(10, 10, 21), (20, 10, 20), (30, 10, 255)])
    cases.append(("threshold_edge", img, None, P, dict(n_all=2, cut=0, n_kept=2, n_desc=0, kept=[(10, 10, 20), (30, 10, 254)])))
    cases.append(("threshold_clamped_high", img, None, dict(P, threshold=1000), dict(n_all=0, cut=0, n_kept=0, n_desc=0, kept=[])))
    img = dots(60, 40, [(10, 10, 0), (20, 10, 179), (30, 10, 180)], bg=200)
    cases.append(("dark_on_bright", img, None, P, dict(n_all=2, cut=0, n_kept=2, n_desc=0, kept=[(10, 10, 199), (20, 10, 20)])))
    return cases


def events(img, excl, threshold, retain, radius):
    """which of the situations the campaign must reach occur in this case -> set of names"""
    img = np.ascontiguousarray(img, np.uint8)
    h, w = img.shape
    ev = set()
    s = np.maximum(score_map(img, threshold), 0)
    if w >= 7 and h >= 7:
        eq = (s[:, :-1] > 0) & (s[:, :-1] == s[:, 1:])
        if eq.any():
            ys, xs = np.nonzero(eq)
            p = np.pad(s, 1)
            for x, y in zip(xs[:64], ys[:64]):                          # a pair that nothing else would have removed
                a = p[y:y + 3, x:x + 3].copy(); a[1, 1] = 0; a[1, 2] = 0
                b = p[y:y + 3, x + 1:x + 4].copy(); b[1, 1] = 0; b[1, 0] = 0
                if a.max() < s[y, x] and b.max() < s[y, x]:
                    ev.add("nms_tie_kills_both")
    xs, ys, sc = corners(img, threshold)
    if (xs == 3).any(): ev.add("corner_col_3")
    if (xs == w - 4).any(): ev.add("corner_col_w-4")
    if (ys == 3).any(): ev.add("corner_row_3")
    if (ys == h - 4).any(): ev.add("corner_row_h-4")
    e = _excl(excl)
    fin = np.isfinite(e).all(axis=1)
    if (~fin).any(): ev.add("non_finite_point")
    frac = e[fin] - np.floor(e[fin])
    half = (frac == 0.5)
    if half.any():
        fl = np.floor(e[fin])[half].astype(np.int64)
        if (fl % 2 == 0).any(): ev.add("half_rounds_down")
        if (fl % 2 != 0).any(): ev.add("half_rounds_up")
    c = centres(excl)
    hw = halfwidths(radius)
    for cx, cy in c:
        inside = 0 <= cx < w and 0 <= cy < h
        touches = cx + radius >= 0 and cx - radius < w and cy + radius >= 0 and cy - radius < h
        if inside:
            if cx - radius < 0: ev.add("clipped_left")
            if cx + radius >= w: ev.add("clipped_right")
            if cy - radius < 0: ev.add("clipped_top")
            if cy + radius >= h: ev.add("clipped_bottom")
        elif touches:
            ev.add("centred_outside")
    if len(c) and len(xs):
        dx = np.abs(xs[:, None].astype(np.int64) - c[None, :, 0]); dy = np.abs(ys[:, None].astype(np.int64) - c[None, :, 1])
        inrow = dy <= radius
        hh = hw[np.where(inrow, dy, 0)]
        covered = inrow & (dx <= hh)
        on_edge = inrow & (dx == hh) & (hh >= 0)
        n_cover = covered.sum(axis=1)
        if ((n_cover == 1) & (covered & on_edge).any(axis=1)).any(): ev.add("removed_by_outermost_pixel")
        if ((n_cover == 0) & (inrow & (dx == hh + 1)).any(axis=1)).any(): ev.add("kept_just_outside")
    ok = ~excluded(xs, ys, excl, radius, w, h)
    r = sc[ok]
    if retain > 0 and len(r) <= retain: ev.add("n_all_le_retain")
    if retain > 0 and len(r) == retain + 1 and (r == np.sort(r)[::-1][retain - 1]).sum() > 1: ev.add("retain_plus_one_tie")
    if retain > 0 and len(r) > retain and len(set(r.tolist())) == 1: ev.add("all_scores_equal")
    if retain == 0 and len(r): ev.add("retain_zero")
    if retain < 0 and len(r): ev.add("retain_negative")
    _, lowest = cut_of(r, retain)
    kx, ky = xs[ok][r >= lowest], ys[ok][r >= lowest]
    if len(kx) and (~((kx >= BORDER) & (kx < w - BORDER) & (ky >= BORDER) & (ky < h - BORDER))).any() and len(r) > max(retain, 0) > 0:
        ev.add("retained_then_border_removed")
    return ev


EVENTS = ("nms_tie_kills_both", "corner_col_3", "corner_col_w-4", "corner_row_3", "corner_row_h-4", "non_finite_point", "half_rounds_down",
          "half_rounds_up", "clipped_left", "clipped_right", "clipped_top", "clipped_bottom", "centred_outside", "removed_by_outermost_pixel",
          "kept_just_outside", "n_all_le_retain", "retain_plus_one_tie", "all_scores_equal", "retain_zero", "retain_negative",
          "retained_then_border_removed")
