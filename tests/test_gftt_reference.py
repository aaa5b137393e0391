"""The numpy restatement of detectGFTT (tests/gftt_ref.py) against the oracle's arithmetic and against literal loops; the host
setMask (ov2_set_mask, no GPU needed) against the oracle's cv::circle."""
import numpy as np
import pytest

from ov2slam_amd import synth
from tests import gftt_ref as R


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("n,seed", [(24, 1), (40, 2), (64, 3)])
def test_eig_of_blur_equals_oracle_cell_mineig(oracle, order, n, seed):
    """on an n x n image the oracle's cell response (blur, then cornerMinEigenVal on the cell = the image) is the restatement's
    whole-image response of the blurred image, bit for bit, in both Sobel dy orders"""
    rng = np.random.default_rng(seed)
    prev, _, _ = synth.frame_pair(2 * n, 2 * n, seed=seed)
    img = np.ascontiguousarray(prev[:n, :n])
    img[rng.integers(0, n, 20), rng.integers(0, n, 20)] = rng.integers(0, 256, 20)
    old = oracle.set_sobel_dy_order(order)
    try:
        ref = oracle.cell_mineig(img, 0, 0, n)
    finally:
        oracle.set_sobel_dy_order(old)
    got = R.mineig(R.blur3(img), order)
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))


@pytest.mark.parametrize("md,maxc", [(35, 1000), (17, 308), (5, 60), (0, 40)])
def test_grid_greedy_equals_literal_loop(md, maxc):
    img, _, _ = synth.frame_pair(320, 200, seed=11)
    eig = R.mineig(img)
    mask = np.full(img.shape, 255, np.uint8)
    xs, ys = R.candidates(eig, mask, 0.0005)
    assert len(xs) > 500
    a = R.greedy(xs, ys, 320, 200, maxc, md)
    b = R.greedy_literal(xs, ys, maxc, md)
    assert a == b


def test_plateau_ties_order_by_offset():
    """equal responses: the later pixel (higher y*w + x) first -- OpenCV 4.x greaterThanPtr"""
    img = np.zeros((48, 64), np.uint8)
    img[8::8, 8::8] = 200                     # isolated equal dots -> equal response peaks
    eig = R.mineig(img)
    xs, ys = R.candidates(eig, np.full(img.shape, 255, np.uint8), 0.01)
    v = eig[ys, xs]
    top = v == v.max()
    assert top.sum() >= 8
    off = ys[top].astype(np.int64) * 64 + xs[top]
    assert np.all(np.diff(off) < 0)
    assert np.all(np.diff(v.astype(np.float64)) <= 0)


def _oracle_mask(oracle, h, w, pts, dist, base=None):
    m = np.full((h, w), 255, np.uint8) if base is None else base.copy()
    for x, y in np.asarray(pts, np.float32).reshape(-1, 2):
        m = oracle.circle_fill0(m, int(np.rint(x)), int(np.rint(y)), dist)
    return m


def test_set_mask_matches_circle_fill0(oracle):
    from ov2slam_amd import frontend
    h, w = 60, 90
    rng = np.random.default_rng(5)
    pts = np.concatenate([
        rng.uniform(-10, 100, (40, 2)),
        [[0.5, 0.5], [1.5, 2.5], [2.5, 3.5], [-0.5, 10], [89.5, 59.5], [45.5, -3.0], [95, 30]],   # half pixels, outside / across the border
    ]).astype(np.float32)
    for dist in (0, 1, 3, 17, 35):
        got = frontend.set_mask(np.full((h, w), 255, np.uint8), pts, dist)
        assert np.array_equal(got, _oracle_mask(oracle, h, w, pts, dist)), dist
    # a strided mask: only the w columns change, the padding keeps its bytes
    buf = np.full((h, w + 7), 9, np.uint8)
    sub = buf[:, :w]
    sub[:] = 255
    frontend.set_mask(sub, pts, 17)
    assert np.array_equal(sub, _oracle_mask(oracle, h, w, pts, 17)) and np.all(buf[:, w:] == 9)


def test_set_mask_round_half_even():
    from ov2slam_amd import frontend
    m = frontend.set_mask(np.full((9, 9), 255, np.uint8), [[2.5, 3.5]], 0)     # cvRound: (2, 4)
    assert list(zip(*np.nonzero(m == 0))) == [(4, 2)]
    m = frontend.set_mask(np.full((9, 9), 255, np.uint8), [[3.5, 2.5]], 0)     # (4, 2)
    assert list(zip(*np.nonzero(m == 0))) == [(2, 4)]


def test_set_mask_invalid_arguments():
    from ov2slam_amd import _lib as L
    import ctypes as C
    lib = L.load()
    m = np.zeros((4, 4), np.uint8)
    p = np.zeros((1, 2), np.float32)
    assert lib.ov2_set_mask(m.ctypes.data_as(C.c_void_p), 4, 4, 3, p.ctypes.data_as(C.c_void_p), 1, 1) == L.OV2_EINVAL
    assert lib.ov2_set_mask(m.ctypes.data_as(C.c_void_p), 4, 4, 4, p.ctypes.data_as(C.c_void_p), 1, -1) == L.OV2_EINVAL
    assert lib.ov2_set_mask(None, 4, 4, 4, p.ctypes.data_as(C.c_void_p), 1, 1) == L.OV2_EINVAL


def test_restatement_two_passes():
    """both branches of the pass-2 rule occur on ordinary frames (the GPU suite relies on it)"""
    img, _, _ = synth.frame_pair(200, 160, seed=3)
    p = R.params(300, 20, 0.01)
    info = {}
    a = R.detect_gftt(img, np.zeros((0, 2)), None, -1, p, subpix=False, info=info)
    assert info["pass2"] and len(a) > 0
    b = R.detect_gftt(img, np.zeros((0, 2)), None, 10, p, subpix=False, info=info)
    assert not info["pass2"] and len(b) == 10
    assert np.array_equal(a[:len(b)], b)          # the same greedy prefix


def test_cpp_runner_compiles_against_fake_opencv(tmp_path):
    """tests/cpp/gftt_run.cpp -- the C++ adapter's detectGFTT and the reference's own FeatureExtractor() / detectGFTT signature in
    ov2slam_amd/host/verbatim.hpp -- compiles and links with -DOV2_WITH_OPENCV against the stand-in tests/fake_opencv (no GPU needed)"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    libdir = os.path.join(root, "ov2slam_amd")
    r = subprocess.run(["g++", "-std=c++17", "-O0", "-Wall", "-Werror", "-DOV2_WITH_OPENCV", "-I" + os.path.join(root, "tests", "fake_opencv"),
                        os.path.join(root, "tests", "cpp", "gftt_run.cpp"), "-o", str(tmp_path / "gftt_run"), "-L", libdir, "-lov2slam_hip",
                        "-Wl,-rpath," + libdir], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
