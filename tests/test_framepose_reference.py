"""tests/framepose_ref.py against the library's host-only sampler: the numpy restatement of the draw gives the integers of
ov2_p3p_draw_samples (the device draw of csrc/framepose.hip is held to the same function on the GPU), and pose_set is the predicate
of the header."""
import numpy as np
import pytest

from ov2slam_amd import pose
from tests import framepose_ref as F

SEEDS = (0, 77, 0xFEDCBA9876543210)


@pytest.mark.parametrize("n", [4, 5, 37, 64, 308])
@pytest.mark.parametrize("rows", [0, 1, 200])
def test_numpy_draw_equals_the_library(n, rows):
    for seed in SEEDS:
        got, want = F.draw_samples(seed, n, rows), pose.draw_samples(seed, n, rows)
        assert got.shape == want.shape == (rows, 4)
        assert np.array_equal(got, want), (seed, n, rows)
        if rows:
            assert got.min() >= 0 and got.max() < n
            assert all(len(set(r)) == 4 for r in got.tolist())
        if n == 4:
            assert all(sorted(r) == [0, 1, 2, 3] for r in got.tolist())


def test_remainder_from_32_bit_pieces_is_the_64_bit_remainder():
    """the device forms z % m as ((hi % m) * (2^32 % m) + lo % m) % m with 32-bit operations; every term stays below 2^23"""
    rng = np.random.default_rng(3)
    for m in (4, 5, 37, 64, 308, 2047, 2048):
        two32 = (0xFFFFFFFF % m + 1) % m
        assert two32 == (1 << 32) % m
        for z in [0, (1 << 64) - 1, (1 << 32) - 1, 1 << 32] + [int(v) for v in rng.integers(0, 1 << 63, 200, dtype=np.int64)]:
            hi, lo = z >> 32, z & 0xFFFFFFFF
            t = (hi % m) * two32 + lo % m
            assert t < (1 << 23) and t % m == z % m


def test_pose_set_is_the_header_predicate():
    status = np.array([1, 0, 3, 1, 2, 1, 5, 1], np.uint8)          # bit 0 tracked, bit 1 went through the retry; higher bits ignored
    is3d = np.array([1, 1, 1, 0, 1, 2, 1, 1], np.uint8)
    assert F.pose_set(status, is3d, 8).tolist() == [0, 5, 6, 7]
    assert F.pose_set(status, is3d, 6).tolist() == [0, 5]
    assert F.pose_set(status, is3d, 0).tolist() == []


@pytest.mark.parametrize("n", [4, 5, 16, 37, 308])
def test_the_device_scheme_gives_the_sequential_table(n):
    """rows drawn 64 at a time from the counters they start at if nothing before them rejects, accepted up to the first rejection:
    the sequential table, at sizes where nearly every row rejects (4, 5) and where few do"""
    for seed in SEEDS:
        for rows in (1, 63, 64, 65, 200):
            assert np.array_equal(F.draw_samples_by_lanes(seed, n, rows), pose.draw_samples(seed, n, rows)), (seed, n, rows)
    assert np.array_equal(F.draw_samples_by_lanes(7, n, 40, lanes=3), pose.draw_samples(7, n, 40))
