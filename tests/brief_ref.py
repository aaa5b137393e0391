"""numpy restatement of FeatureExtractor::describeBRIEF (OpenCV contrib BriefDescriptorExtractor, 32 bytes, no orientation): the
CPU reference the BRIEF tests compare the HIP kernel with.  Exact integer arithmetic on an OpenCV-style CV_32S integral image, so
it does not depend on how the kernel sums.  Test-only: the product never imports it.

Rules (DESIGN.md "BRIEF"; restated from the public OpenCV source, to be confirmed on an OpenCV build):
  valid   28 <= rint(x) < W-28 and 28 <= rint(y) < H-28 (half to even; non-finite never)
  centre  cx = (int)((double)x + 0.5), cy alike
  S       9x9 box sum centred at (cy+dy, cx+dx); pixels outside the image count 0 (the odd-size corner case, where OpenCV reads
          past its integral image, is defined this way)
  bit t   S(ay, ax) < S(by, bx); byte j = bits 8j..8j+7, MSB first; a rejected point's row is zero
"""
import numpy as np

BORDER = 28
HALF_KERNEL = 4


def border_valid(pts, w, h):
    """runByImageBorder(keypoints, Size(w, h), 28) as a per-point flag"""
    p = np.asarray(pts, np.float32).reshape(-1, 2)
    with np.errstate(invalid="ignore"):
        r = np.rint(p)                                   # half to even, like saturate_cast<int>(float)
        ok = np.isfinite(p).all(axis=1)
        ok &= (r[:, 0] >= BORDER) & (r[:, 0] < w - BORDER) & (r[:, 1] >= BORDER) & (r[:, 1] < h - BORDER)
    return ok


def centres(pts):
    p = np.asarray(pts, np.float32).reshape(-1, 2).astype(np.float64)
    return np.trunc(p + 0.5)                               # (int)(pt + 0.5): truncation (every surviving point is positive)


def integral(img):
    """CV_32S integral image of the image zero-padded by one row and column: (H+2) x (W+2), sum[r, c] = sum of rows < r, cols < c"""
    img = np.asarray(img, np.int64)
    H, W = img.shape
    s = np.zeros((H + 2, W + 2), np.int64)
    s[1:H + 1, 1:W + 1] = img.cumsum(0).cumsum(1)
    s[H + 1, 1:W + 1] = s[H, 1:W + 1]
    s[:, W + 1] = s[:, W]
    return s


def describe(img, pts, pattern):
    """-> (desc (n, 32) uint8, valid (n,) bool)"""
    img = np.asarray(img, np.uint8)
    H, W = img.shape
    pattern = np.asarray(pattern, np.int64).reshape(256, 4)
    valid = border_valid(pts, W, H)
    n = len(valid)
    desc = np.zeros((n, 32), np.uint8)
    if not valid.any():
        return desc, valid
    c = centres(np.asarray(pts, np.float32).reshape(-1, 2)[valid]).astype(np.int64)
    cx, cy = c[:, 0], c[:, 1]
    s = integral(img)

    def smoothed(dy, dx):                          # smoothedSum: four reads of the integral image
        y, x = cy + dy, cx + dx
        return (s[y + HALF_KERNEL + 1, x + HALF_KERNEL + 1] - s[y + HALF_KERNEL + 1, x - HALF_KERNEL]
                - s[y - HALF_KERNEL, x + HALF_KERNEL + 1] + s[y - HALF_KERNEL, x - HALF_KERNEL])

    bits = np.zeros((len(cx), 256), np.uint8)
    for t in range(256):
        ay, ax, by, bx = pattern[t]
        bits[:, t] = smoothed(ay, ax) < smoothed(by, bx)
    desc[valid] = np.packbits(bits, axis=1, bitorder="big")
    return desc, valid


def describe_scalar(img, pts, pattern):
    """The same rules as plain loops over the pixels (no integral image, no vectorisation): the restatement's own check."""
    img = np.asarray(img, np.uint8)
    H, W = img.shape
    pattern = np.asarray(pattern).reshape(256, 4)
    out, ok = [], []
    for x, y in np.asarray(pts, np.float32).reshape(-1, 2):
        d = bytearray(32)
        fx, fy = float(x), float(y)
        good = np.isfinite(fx) and np.isfinite(fy)
        if good:
            rx, ry = round(fx), round(fy)                 # Python rounds half to even
            good = BORDER <= rx < W - BORDER and BORDER <= ry < H - BORDER
        if good:
            cx, cy = int(fx + 0.5), int(fy + 0.5)

            def S(dy, dx):
                tot = 0
                for yy in range(cy + dy - 4, cy + dy + 5):
                    for xx in range(cx + dx - 4, cx + dx + 5):
                        if 0 <= yy < H and 0 <= xx < W:
                            tot += int(img[yy, xx])
                return tot
            for t in range(256):
                ay, ax, by, bx = (int(v) for v in pattern[t])
                if S(ay, ax) < S(by, bx):
                    d[t // 8] |= 1 << (7 - t % 8)
        out.append(bytes(d))
        ok.append(good)
    return np.frombuffer(b"".join(out), np.uint8).reshape(-1, 32).copy(), np.array(ok, bool)


def describe_stack(imgs, pts, pattern):
    """describe() of the same keypoints on every image of an (n, H, W) stack -> (desc (n, k, 32), valid (k,))"""
    imgs = np.asarray(imgs, np.uint8)
    n, H, W = imgs.shape
    pattern = np.asarray(pattern, np.int64).reshape(256, 4)
    valid = border_valid(pts, W, H)
    desc = np.zeros((n, len(valid), 32), np.uint8)
    if not valid.any():
        return desc, valid
    c = centres(np.asarray(pts, np.float32).reshape(-1, 2)[valid]).astype(np.int64)
    cx, cy = c[:, 0], c[:, 1]
    s = np.zeros((n, H + 2, W + 2), np.int64)
    s[:, 1:H + 1, 1:W + 1] = imgs.astype(np.int64).cumsum(1).cumsum(2)
    s[:, H + 1, 1:W + 1] = s[:, H, 1:W + 1]
    s[:, :, W + 1] = s[:, :, W]

    def smoothed(dy, dx):
        y, x = cy + dy, cx + dx
        return (s[:, y + HALF_KERNEL + 1, x + HALF_KERNEL + 1] - s[:, y + HALF_KERNEL + 1, x - HALF_KERNEL]
                - s[:, y - HALF_KERNEL, x + HALF_KERNEL + 1] + s[:, y - HALF_KERNEL, x - HALF_KERNEL])

    bits = np.zeros((n, len(cx), 256), np.uint8)
    for t in range(256):
        ay, ax, by, bx = pattern[t]
        bits[:, :, t] = smoothed(ay, ax) < smoothed(by, bx)
    desc[:, valid] = np.packbits(bits, axis=2, bitorder="big")
    return desc, valid
