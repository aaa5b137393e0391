"""cv::remap for CV_8UC1 / INTER_LINEAR / BORDER_CONSTANT 0 -- OpenCV's own C++ path, RESTATED in numpy (integers only) as the
reference of ov2_rectify_* (include/ov2slam_hip.h); not pinned against an OpenCV build.  Also the maps the tests feed it:
a plain float64 pinhole rad-tan inverse mapping with a rotation, emitted in both forms the reference creates (test input, not a
claim about cv::initUndistortRectifyMap's bits), and the conversion OV2_MAP_F32 -> normalised map."""
import numpy as np

INTER_BITS = 5
INTER_TAB_SIZE = 1 << INTER_BITS          # 32
INTER_REMAP_COEF_BITS = 15
INTER_REMAP_COEF_SCALE = 1 << INTER_REMAP_COEF_BITS


def normalise_f32(map_x, map_y):
    """OV2_MAP_F32 -> (ixy (h, w, 2) int16, ab (h, w) uint16): per pixel sx = cvRound(x * 32.f) (the float product is exact, the
    rounding to nearest with ties to even), ix = saturate_cast<short>(sx >> 5), a = sx & 31 (arithmetic shift and two's complement:
    negative coordinates floor); iy, b likewise; ab = b * 32 + a -- the OV2_MAP_FIXED form (CV_16SC2 + CV_16UC1)."""
    mx = np.asarray(map_x, np.float32); my = np.asarray(map_y, np.float32)
    assert mx.shape == my.shape and mx.ndim == 2
    assert np.isfinite(mx).all() and np.isfinite(my).all()
    px = mx * np.float32(INTER_TAB_SIZE); py = my * np.float32(INTER_TAB_SIZE)
    assert px.dtype == np.float32 and (np.abs(px) < 2.0 ** 31).all() and (np.abs(py) < 2.0 ** 31).all()
    sx = np.rint(px.astype(np.float64)).astype(np.int64)          # np.rint: ties to even, like cvRound / __float2int_rn
    sy = np.rint(py.astype(np.float64)).astype(np.int64)
    ix = np.clip(sx >> INTER_BITS, -32768, 32767).astype(np.int16)
    iy = np.clip(sy >> INTER_BITS, -32768, 32767).astype(np.int16)
    ab = ((sy & (INTER_TAB_SIZE - 1)) * INTER_TAB_SIZE + (sx & (INTER_TAB_SIZE - 1))).astype(np.uint16)
    return np.stack([ix, iy], axis=-1), ab


def remap_fixed(img, ixy, ab):
    """The restatement, vectorised.  With p00, p01, p10, p11 the source pixels at (ix, iy), (ix+1, iy), (ix, iy+1), (ix+1, iy+1) and
    every tap outside the source image counted as 0 (OpenCV's inlier, partly-outside and fully-outside branches in one):

        out = (p00*(32-a)*(32-b)*32 + p01*a*(32-b)*32 + p10*(32-a)*b*32 + p11*a*b*32 + (1 << 14)) >> 15

    The weights are OpenCV's BilinearTab_i exactly for every (a, b) != (0, 0): the products are integers and sum to 32768.  At
    (0, 0) OpenCV's short table cannot hold 32768: it holds 32767, and the missing 1 goes to another tap (the fix-up of
    initInterTab2D moves it to a neighbouring table entry).  For 8-bit pixels both give p00 exactly: with p the pixel under the
    32767 and p' the one under the 1, 32767*p + p' + 16384 = 32768*p + (16384 + p' - p) and 16384 + p' - p lies in
    [16129, 16639], inside [0, 32768) for p, p' <= 255 -- so the sum lies in [32768*p, 32768*(p+1)) and >> 15 gives p, which is
    what weight 32768 on p00 gives ((32768*p + 16384) >> 15 = p).  tests/test_remap_reference.py checks all 256 x 256 pairs."""
    img = np.asarray(img, np.uint8)
    h, w = img.shape
    ix = ixy[..., 0].astype(np.int64); iy = ixy[..., 1].astype(np.int64)
    a = (ab.astype(np.int64) & 31); b = (ab.astype(np.int64) >> 5)
    assert (ab < 1024).all()

    def tap(x, y):
        ok = (x >= 0) & (x < w) & (y >= 0) & (y < h)
        v = img[np.clip(y, 0, h - 1), np.clip(x, 0, w - 1)].astype(np.int64)
        return np.where(ok, v, 0)

    p00, p01, p10, p11 = tap(ix, iy), tap(ix + 1, iy), tap(ix, iy + 1), tap(ix + 1, iy + 1)
    acc = (p00 * (32 - a) * (32 - b) * 32 + p01 * a * (32 - b) * 32 + p10 * (32 - a) * b * 32 + p11 * a * b * 32
           + (1 << (INTER_REMAP_COEF_BITS - 1))) >> INTER_REMAP_COEF_BITS
    assert acc.min() >= 0 and acc.max() <= 255
    return acc.astype(np.uint8)


def remap_f32(img, map_x, map_y):
    ixy, ab = normalise_f32(map_x, map_y)
    return remap_fixed(img, ixy, ab)


def remap(img, form, map1, map2):
    """form: "f32" (map1 = x, map2 = y, float32) or "fixed" (map1 = (h, w, 2) int16, map2 = (h, w) uint16)"""
    return remap_f32(img, map1, map2) if form == "f32" else remap_fixed(img, np.asarray(map1, np.int16), np.asarray(map2, np.uint16))


def both_forms(map_x, map_y):
    """float maps -> {"f32": (x, y), "fixed": (ixy, ab)}: the fixed form is what cv::convertMaps makes of the float one"""
    mx = np.ascontiguousarray(map_x, np.float32); my = np.ascontiguousarray(map_y, np.float32)
    ixy, ab = normalise_f32(mx, my)
    return {"f32": (mx, my), "fixed": (np.ascontiguousarray(ixy), np.ascontiguousarray(ab))}


# ---- map generators (test input) -------------------------------------------------------------------------------------------

def _rot(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def radtan_maps(w, h, K, D, R=None, newK=None):
    """Inverse mapping of a pinhole rad-tan camera, float64: destination pixel (u, v) -> normalised ray through newK -> rotated by
    R^-1 -> distorted with D = (k1, k2, p1, p2) -> source pixel through K.  -> (map_x, map_y) float32"""
    fx, fy, cx, cy = K
    nfx, nfy, ncx, ncy = newK if newK is not None else K
    k1, k2, p1, p2 = D
    iR = np.linalg.inv(R if R is not None else np.eye(3))
    u, v = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    x, y = (u - ncx) / nfx, (v - ncy) / nfy
    X = iR[0, 0] * x + iR[0, 1] * y + iR[0, 2]
    Y = iR[1, 0] * x + iR[1, 1] * y + iR[1, 2]
    W = iR[2, 0] * x + iR[2, 1] * y + iR[2, 2]
    x, y = X / W, Y / W
    r2 = x * x + y * y
    kr = 1 + k1 * r2 + k2 * r2 * r2
    xd = x * kr + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
    yd = y * kr + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
    return (fx * xd + cx).astype(np.float32), (fy * yd + cy).astype(np.float32)


def identity_maps(w, h):
    u, v = np.meshgrid(np.arange(w, dtype=np.float32), np.arange(h, dtype=np.float32))
    return u, v


def shift_maps(w, h, dx, dy):
    """out(x, y) = img(x + dx, y + dy)"""
    u, v = identity_maps(w, h)
    return u + np.float32(dx), v + np.float32(dy)


def euroc_like_maps(w, h):
    """k1 -0.28, k2 0.07, small p1 / p2, a 1.5 degree rotation (EuRoC's cam0 is about this distorted)"""
    f = 0.61 * w
    K = (f, f * 0.997, 0.49 * w, 0.52 * h)
    return radtan_maps(w, h, K, (-0.28, 0.07, 2e-4, 2e-5), _rot(np.deg2rad(0.4), np.deg2rad(-0.3), np.deg2rad(1.5)))


def wild_maps(w, h):
    """25 degree in-plane rotation about the image centre, scale 1.3, an offset: all four borders and all four corners of the
    destination leave the source, with coordinates below -1 and beyond w, h"""
    u, v = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    c, s = np.cos(np.deg2rad(25.0)) * 1.3, np.sin(np.deg2rad(25.0)) * 1.3
    du, dv = u - (w - 1) / 2.0, v - (h - 1) / 2.0
    mx = c * du - s * dv + (w - 1) / 2.0 + 0.37
    my = s * du + c * dv + (h - 1) / 2.0 - 0.21
    return mx.astype(np.float32), my.astype(np.float32)


TIES = (2 + 1 / 64., 2 + 3 / 64., 5 + 1 / 64., 5 + 3 / 64.)      # k + 1/64 -> k (32k + 0.5 rounds to even), k + 3/64 -> k + 2/32


def edge_values(n):
    """source coordinates around both ends of an axis of n pixels, and the tie values"""
    return [-1.5, -1.0, -31 / 32., -0.5, -1 / 64., 0.0, 1 / 64., n - 2.0, n - 1 - 1 / 32., n - 1.0, n - 0.5, float(n)] + list(TIES)


def edge_maps(w, h):
    """A hand-made map that enumerates edge_values(w) x edge_values(h): destination pixel (x, y) reads source
    (ex[x % len(ex)], ey[(y + x // len(ex)) % len(ey)]), so every pair occurs once the destination has len(ex) * len(ey) pixels"""
    ex, ey = np.array(edge_values(w), np.float32), np.array(edge_values(h), np.float32)
    u, v = np.meshgrid(np.arange(w), np.arange(h))
    mx = ex[u % len(ex)]
    my = ey[(v + u // len(ex)) % len(ey)]
    return np.ascontiguousarray(mx), np.ascontiguousarray(my)
