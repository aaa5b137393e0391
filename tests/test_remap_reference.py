"""tests/remap_ref.py -- the restatement of cv::remap (CV_8UC1, INTER_LINEAR, BORDER_CONSTANT 0) the device rectification is held
against -- checked on the CPU two independent ways: a per-pixel scalar loop written with OpenCV's three branches, and the exact
bilinear value at the 1/32-quantised coordinate in rational arithmetic."""
from fractions import Fraction

import numpy as np
import pytest

from tests import remap_ref as R


def _scalar_three_branches(img, ixy, ab):
    """remapBilinear's structure for one channel, BORDER_CONSTANT 0: a pixel whose 2 x 2 footprint lies inside the source (inlier),
    one whose footprint lies wholly outside (constant), one in between (each tap fetched or replaced by the constant)"""
    h, w = img.shape
    dh, dw = ab.shape
    out = np.zeros((dh, dw), np.uint8)
    for y in range(dh):
        for x in range(dw):
            sx, sy = int(ixy[y, x, 0]), int(ixy[y, x, 1])
            a, b = int(ab[y, x]) & 31, int(ab[y, x]) >> 5
            wt = [(32 - a) * (32 - b) * 32, a * (32 - b) * 32, (32 - a) * b * 32, a * b * 32]
            if 0 <= sx < w - 1 and 0 <= sy < h - 1:                                      # inlier
                v = [int(img[sy, sx]), int(img[sy, sx + 1]), int(img[sy + 1, sx]), int(img[sy + 1, sx + 1])]
            elif sx >= w or sx + 1 < 0 or sy >= h or sy + 1 < 0:                         # fully outside
                out[y, x] = 0
                continue
            else:                                                                        # partly outside
                v = []
                for (yy, xx) in ((sy, sx), (sy, sx + 1), (sy + 1, sx), (sy + 1, sx + 1)):
                    v.append(int(img[yy, xx]) if 0 <= xx < w and 0 <= yy < h else 0)
            out[y, x] = (v[0] * wt[0] + v[1] * wt[1] + v[2] * wt[2] + v[3] * wt[3] + (1 << 14)) >> 15
    return out


def _fraction_exact(img, ixy, ab):
    """floor(exact bilinear value at (ix + a/32, iy + b/32) + 1/2), zero outside the image"""
    h, w = img.shape
    dh, dw = ab.shape
    out = np.zeros((dh, dw), np.uint8)

    def px(xx, yy):
        return Fraction(int(img[yy, xx])) if 0 <= xx < w and 0 <= yy < h else Fraction(0)

    for y in range(dh):
        for x in range(dw):
            sx, sy = int(ixy[y, x, 0]), int(ixy[y, x, 1])
            fa, fb = Fraction(int(ab[y, x]) & 31, 32), Fraction(int(ab[y, x]) >> 5, 32)
            v = ((1 - fa) * (1 - fb) * px(sx, sy) + fa * (1 - fb) * px(sx + 1, sy) + (1 - fa) * fb * px(sx, sy + 1) + fa * fb * px(sx + 1, sy + 1))
            out[y, x] = (v + Fraction(1, 2)).__floor__()
    return out


@pytest.fixture(scope="module", params=[(83, 37), (64, 48)])
def case(request):
    """image, a map that mixes smooth distortion, everything-leaves-the-image and the hand-made edge values, its normalised form and
    the vectorised reference's answer (computed once, shared)"""
    w, h = request.param
    rng = np.random.default_rng(w * 1000 + h)
    img = rng.integers(0, 256, (h, w), dtype=np.uint8)
    maps = []
    for mx, my in (R.wild_maps(w, h), R.edge_maps(w, h), R.euroc_like_maps(w, h)):
        maps.append(R.normalise_f32(mx, my))
    ixy = np.concatenate([m[0] for m in maps], axis=0)
    ab = np.concatenate([m[1] for m in maps], axis=0)
    return img, ixy, ab, R.remap_fixed(img, ixy, ab)


def test_vectorised_equals_scalar_three_branches(case):
    img, ixy, ab, ref = case
    got = _scalar_three_branches(img, ixy, ab)
    assert np.array_equal(got, ref)
    h, w = img.shape
    sx, sy = ixy[..., 0].astype(int), ixy[..., 1].astype(int)
    inl = (sx >= 0) & (sx < w - 1) & (sy >= 0) & (sy < h - 1)
    out = (sx >= w) | (sx + 1 < 0) | (sy >= h) | (sy + 1 < 0)
    assert inl.any() and out.any() and (~inl & ~out).any()          # all three branches were taken


def test_vectorised_equals_exact_bilinear(case):
    img, ixy, ab, ref = case
    assert np.array_equal(_fraction_exact(img, ixy, ab), ref)


def test_identity_shift_and_all_outside():
    rng = np.random.default_rng(5)
    w, h = 83, 37
    img = rng.integers(0, 256, (h, w), dtype=np.uint8)
    assert np.array_equal(R.remap_f32(img, *R.identity_maps(w, h)), img)
    sh = R.remap_f32(img, *R.shift_maps(w, h, 3, -2))               # out(x, y) = img(x + 3, y - 2)
    exp = np.zeros_like(img)
    exp[2:, :w - 3] = img[:h - 2, 3:]
    assert np.array_equal(sh, exp)
    for dx, dy in ((w + 5, 0), (-w - 5, 0), (0, h + 1), (0, -h - 1), (1e6, -1e6)):
        assert not R.remap_f32(img, *R.shift_maps(w, h, dx, dy)).any()
    # the fixed form of the same maps gives the same image
    f = R.both_forms(*R.shift_maps(w, h, 3, -2))
    assert np.array_equal(R.remap(img, "fixed", *f["fixed"]), exp) and np.array_equal(R.remap(img, "f32", *f["f32"]), exp)


def test_ties_round_to_even():
    k = np.arange(0, 40, dtype=np.float32)
    one = np.zeros((1, len(k)), np.float32)
    ixy, ab = R.normalise_f32((k + np.float32(1 / 64.))[None], one)          # 32 k + 0.5 -> 32 k (even)
    assert np.array_equal(ixy[0, :, 0], k.astype(np.int16)) and np.array_equal(ab[0] & 31, np.zeros(len(k), np.uint16))
    ixy, ab = R.normalise_f32((k + np.float32(3 / 64.))[None], one)          # 32 k + 1.5 -> 32 k + 2 (even)
    assert np.array_equal(ixy[0, :, 0], k.astype(np.int16)) and np.array_equal(ab[0] & 31, np.full(len(k), 2, np.uint16))
    ixy, ab = R.normalise_f32(one, (k + np.float32(1 / 64.))[None])          # the same on the y axis
    assert np.array_equal(ixy[0, :, 1], k.astype(np.int16)) and np.array_equal(ab[0] >> 5, np.zeros(len(k), np.uint16))


def test_negative_coordinates_floor():
    v = np.array([[-1 / 64., -0.5, -1.0, -1.5]], np.float32)
    ixy, ab = R.normalise_f32(v, v)
    # -1/64: -0.5 -> 0 (even) -> (0, 0);  -0.5: -16 -> (-1, 16);  -1: -32 -> (-1, 0);  -1.5: -48 -> (-2, 16)
    assert ixy[0, :, 0].tolist() == [0, -1, -1, -2] and (ab[0] & 31).tolist() == [0, 16, 0, 16]
    assert ixy[0, :, 1].tolist() == [0, -1, -1, -2] and (ab[0] >> 5).tolist() == [0, 16, 0, 16]
    img = np.array([[200, 100], [50, 10]], np.uint8)
    out = R.remap_f32(img, v, v)
    # (-0.5, -0.5): only p11 = img[0, 0] is inside, weight 1/4 -> floor(50 + 0.5) = 50; (-1, -1): p11 = img[0, 0] with weight 0
    assert out[0].tolist() == [200, 50, 0, 0]


def test_weight_table_at_zero_zero_gives_p00_for_8_bit_pixels():
    p00, p11 = np.meshgrid(np.arange(256, dtype=np.int64), np.arange(256, dtype=np.int64), indexing="ij")
    restated = (p00 * 32768 + (1 << 14)) >> 15                      # the expression of remap_fixed at (a, b) = (0, 0)
    opencv = (p00 * 32767 + p11 * 1 + (1 << 14)) >> 15              # BilinearTab_i[0]: 32767 and the fix-up's 1 on another tap
    assert np.array_equal(restated, p00) and np.array_equal(opencv, p00)
    s = p00 * 32767 + p11 + (1 << 14)
    assert (s >= 32768 * p00).all() and (s < 32768 * (p00 + 1)).all()
