"""numpy restatement of FeatureExtractor::detectGFTT (the reference's src/feature_extractor.cpp:104-221) as
include/ov2slam_hip.h specifies it: cv::goodFeaturesToTrack (OpenCV 4.x, min-eigenvalue response, blockSize 3, gradSize 3)
once or twice per image, with setMask's filled circles.  Element-wise float32 steps, the double sliding column sum walked row by
row; circles from oracle.circle_fill0, cornerSubPix from oracle.corner_subpix."""
import numpy as np

from oracle import oracle as O

F1 = np.float32(1.0 / (4.0 * 3.0 * 255.0))
F0 = np.float32(2.0 * (1.0 / (4.0 * 3.0 * 255.0)))


def reflect101(i, n):
    if n == 1:
        return 0
    while i < 0 or i >= n:
        i = -i if i < 0 else 2 * n - 2 - i
    return i


def _ridx(n):
    return np.array([reflect101(i, n) for i in range(-1, n + 1)], np.int64)


def mineig(img, dy_order=O.SOBEL_DY_OPENCV_ROWFILTER):
    """cornerMinEigenVal(img, eig, 3, 3), REFLECT_101 at the image border -> (h, w) float32"""
    I = np.asarray(img, np.int32)
    h, w = I.shape
    ry, rx = _ridx(h), _ridx(w)
    P = I[ry][:, rx]                                          # (h+2, w+2): pixel rows / columns -1 .. n
    f32 = np.float32
    a0 = (P[:-2, 2:] - P[:-2, :-2]).astype(f32)
    a1 = (P[1:-1, 2:] - P[1:-1, :-2]).astype(f32)
    a2 = (P[2:, 2:] - P[2:, :-2]).astype(f32)
    dx = (a0 + a2) * F1 + a1 * F0
    if dy_order == O.SOBEL_DY_EXACT_SUM:
        s0 = (P[:-2, :-2] + 2 * P[:-2, 1:-1] + P[:-2, 2:]).astype(f32)
        s2 = (P[2:, :-2] + 2 * P[2:, 1:-1] + P[2:, 2:]).astype(f32)
        dy = (s2 - s0) * F1
    else:
        s0 = (P[:-2, :-2].astype(f32) * F1 + P[:-2, 1:-1].astype(f32) * F0) + P[:-2, 2:].astype(f32) * F1
        s2 = (P[2:, :-2].astype(f32) * F1 + P[2:, 1:-1].astype(f32) * F0) + P[2:, 2:].astype(f32) * F1
        dy = s2 - s0
    cov = np.empty((h, w, 3), f32)
    for ch, v in enumerate((dx * dx, dx * dy, dy * dy)):
        V = v[:, rx].astype(np.float64)                       # RowSum<float, double>, ksize 3
        R = ((V[:, :-2] + V[:, 1:-1]) + V[:, 2:])[ry]         # rows -1 .. h (reflected)
        SUM = np.zeros(w, np.float64)
        SUM += R[0]
        SUM += R[1]
        for y in range(h):                                    # ColumnSum<double, float>
            s = SUM + R[y + 2]
            cov[y, :, ch] = s.astype(f32)
            SUM = s - R[y]
    a = cov[..., 0] * f32(0.5)
    b = cov[..., 1]
    c = cov[..., 2] * f32(0.5)
    return ((a + c) - np.sqrt((a - c) * (a - c) + b * b)).astype(f32)


def blur3(img):
    """GaussianBlur 3x3, sigma 0, 8-bit fixed point (the oracle's default), REFLECT_101"""
    I = np.asarray(img, np.int32)
    h, w = I.shape
    P = I[_ridx(h)][:, _ridx(w)]
    r = P[:, :-2] + 2 * P[:, 1:-1] + P[:, 2:]
    s = r[:-2] + 2 * r[1:-1] + r[2:]
    return ((s + 8) >> 4).astype(np.uint8)


def set_mask(mask, pts, dist):
    """FeatureExtractor::setMask: cv::circle(mask, Point(cvRound(x), cvRound(y)), dist, 0, FILLED) for every point"""
    for x, y in np.asarray(pts, np.float32).reshape(-1, 2):
        if not (abs(x) < 1e7 and abs(y) < 1e7):
            continue
        mask = O.circle_fill0(mask, int(np.rint(x)), int(np.rint(y)), int(dist))
    return mask


def candidates(eig, mask, quality):
    """threshold + dilate + mask -> (x, y) int arrays in the sorted order (value descending, equal values: higher offset first)"""
    h, w = eig.shape
    sel = eig[mask != 0]
    maxval = float(sel.max()) if sel.size else 0.0
    thr = np.float32(maxval * quality)
    t = np.where(eig > thr, eig, np.float32(0))
    c = t[1:-1, 1:-1]
    dil = c.copy()
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            dil = np.maximum(dil, t[1 + dy:h - 1 + dy, 1 + dx:w - 1 + dx])
    ok = (c != 0) & (c == dil) & (mask[1:-1, 1:-1] != 0)
    ys, xs = np.nonzero(ok)
    ys = ys + 1
    xs = xs + 1
    val = t[ys, xs]
    off = ys.astype(np.int64) * w + xs
    order = np.lexsort((-off, -val.astype(np.float64)))
    return xs[order], ys[order]


def greedy(xs, ys, w, h, max_corners, min_distance):
    """featureselect.cpp's grid pass (cell side cvRound(minDistance), 3x3 neighbouring cells)"""
    acc = []
    if min_distance < 1:
        return list(zip(xs[:max_corners].tolist(), ys[:max_corners].tolist()))
    cs = int(round(min_distance))
    gw, gh = (w + cs - 1) // cs, (h + cs - 1) // cs
    grid = {}
    md2 = float(min_distance) ** 2
    for x, y in zip(xs.tolist(), ys.tolist()):
        cx, cy = x // cs, y // cs
        good = True
        for yy in range(max(cy - 1, 0), min(cy + 1, gh - 1) + 1):
            for xx in range(max(cx - 1, 0), min(cx + 1, gw - 1) + 1):
                for (px, py) in grid.get((xx, yy), ()):
                    if (x - px) ** 2 + (y - py) ** 2 < md2:
                        good = False
                        break
                if not good:
                    break
            if not good:
                break
        if good:
            grid.setdefault((cx, cy), []).append((x, y))
            acc.append((x, y))
            if len(acc) == max_corners:
                break
    return acc


def greedy_literal(xs, ys, max_corners, min_distance):
    """the same selection as an O(n^2) loop over the whole accepted list"""
    acc = []
    for x, y in zip(xs.tolist(), ys.tolist()):
        if all((x - px) ** 2 + (y - py) ** 2 >= min_distance ** 2 for px, py in acc):
            acc.append((x, y))
            if len(acc) == max_corners:
                break
    return acc


def gftt_pass(img, eig, mask, max_corners, quality, min_distance, subpix):
    h, w = eig.shape
    xs, ys = candidates(eig, mask, quality)
    pts = np.array(greedy(xs, ys, w, h, max_corners, min_distance), np.float32).reshape(-1, 2)
    if subpix and len(pts):
        pts = O.corner_subpix(img, pts, 3, 30, 0.01)
    return pts, len(xs)


def params(nmaxpts, nmaxdist, dmaxquality):
    """the constructor's derived members (:79-83)"""
    return dict(nmaxpts=int(nmaxpts), nmaxdist=int(nmaxdist), nmindist=int(nmaxdist) // 2,
                dminquality=dmaxquality / 2., dmaxquality=float(dmaxquality))


def detect_gftt(img, cur, roi, nbmax, p, subpix=True, dy_order=O.SOBEL_DY_OPENCV_ROWFILTER, eig=None, info=None):
    """-> (n, 2) float32.  roi None or an (h, w) uint8 mask; p from params().  info (a dict) receives pass2 / ncand."""
    img = np.ascontiguousarray(img, np.uint8)
    h, w = img.shape
    cur = np.asarray(cur, np.float32).reshape(-1, 2)
    if len(cur) >= p["nmaxpts"]:
        return np.zeros((0, 2), np.float32)
    nb2 = nbmax if nbmax != -1 else p["nmaxpts"] - len(cur)
    if eig is None:
        eig = mineig(img, dy_order)
    base = np.full((h, w), 255, np.uint8) if roi is None else np.ascontiguousarray(roi, np.uint8).copy()
    mask = set_mask(base.copy(), cur, p["nmaxdist"])
    pts1, nc1 = gftt_pass(img, eig, mask, nb2, p["dminquality"], p["nmaxdist"], subpix)
    if info is not None:
        info.update(pass2=False, ncand=[nc1])
    if len(pts1) >= 0.66 * nb2 or nb2 < 20:
        return pts1
    mask = set_mask(base.copy(), cur, p["nmindist"])
    mask = set_mask(mask, pts1, p["nmindist"])
    pts2, nc2 = gftt_pass(img, eig, mask, nb2 - len(pts1), p["dmaxquality"], p["nmindist"], subpix)
    if info is not None:
        info.update(pass2=True, ncand=[nc1, nc2])
    return np.concatenate([pts1, pts2]).astype(np.float32)
