"""tests/p3p_ref.py, the numpy specification of the device P3P pose search, against ground truth and against its own written
rules (no GPU): noise-free recovery, the solver's properties, planted outliers under both loops, one case per loop quirk, the
clamp of the distance, and the sample generator (known answers, and ov2_p3p_draw_samples -- host only -- gives the same integers)."""
import numpy as np
import pytest

from tests import p3p_ref as R

TH = R.threshold_of(3.0, 460.0, 460.0)


def test_threshold_expression():
    """1 - cos(atan(3 / 460)) = 2.1266e-5, the quotient being a float as in the reference (errth and focal are floats)"""
    assert TH == 1.0 - np.cos(np.arctan(np.float64(np.float32(3.0) / np.float32(460.0)))) and 2.12e-5 < TH < 2.13e-5


def test_noise_free_recovery():
    """200 random 4-point scenes: the hypothesis the fourth point picks is the ground truth (bound of the issue: 1e-8)"""
    rng = np.random.default_rng(0)
    worst = 0.0
    for _ in range(200):
        bv, X, Rw, C, _ = R.make_scene(rng, 4)
        m = R.hypothesis([0, 1, 2, 3], bv, X)
        assert m is not None
        worst = max(worst, np.abs(m[:, :3] - Rw).max(), np.abs(m[:, 3] - C).max())
    print("worst |R - R_gt|, |C - C_gt|: %.3g" % worst)
    assert worst <= 1e-8


def _solutions(seed=1, scenes=100):
    rng = np.random.default_rng(seed)
    for _ in range(scenes):
        bv, X, Rw, C, _ = R.make_scene(rng, 3)
        yield bv, X, Rw, C, R.kneip(bv, X)


def test_every_accepted_solution_is_a_rotation_and_the_truth_is_among_them():
    """a product of three orthogonal matrices: orthogonal with determinant +1 to 1e-12, whatever the root; and in every scene
    one accepted solution reproduces all three bearings (d is quadratic in the angular error: 1e-12 is rounding level)"""
    nsol = 0
    for bv, X, Rw, C, sols in _solutions():
        assert 1 <= len(sols) <= 4
        for Rm, Cm in sols:
            nsol += 1
            assert np.abs(Rm @ Rm.T - np.eye(3)).max() <= 1e-12 and abs(np.linalg.det(Rm) - 1.0) <= 1e-12
        assert min(R.distances(Rm, Cm, bv, X).max() for Rm, Cm in sols) <= 1e-12
    assert nsol > 150          # two solutions are the rule


def test_every_accepted_solution_reproduces_its_three_bearings():
    """d at rounding level (1e-12, p3p_ref.BEARING_TOL) for every solution the solver returns.  The quartic's accepted roots
    alone do not have this property (553 of the 606 of these scenes do; 20 are roots of the mirrored configuration that squaring
    sin(theta) away adds, 33 put the centre beyond point 1 or 2): the specification makes it part of what a solution is."""
    bad, worst, nsol, nroots = 0, 0.0, 0, 0
    for bv, X, Rw, C, sols in _solutions(scenes=300):
        with np.errstate(all="ignore"):
            nroots += len(R.accept_roots(R.quartic(bv, X)[0]))
        for Rm, Cm in sols:
            d = R.distances(Rm, Cm, bv, X).max()
            nsol += 1
            bad += int(d > 1e-12)
            worst = max(worst, d)
    print("accepted roots %d, solutions %d, not reproducing their bearings %d, largest d %.3g" % (nroots, nsol, bad, worst))
    assert bad == 0
    assert nsol >= 500 and nroots - nsol >= 20        # the rule removes something, and not much


@pytest.mark.parametrize("mode", [R.LMEDS, R.RANSAC], ids=["lmeds", "ransac"])
@pytest.mark.parametrize("n,frac,seed", [(60, 0.25, 3), (130, 0.3, 4), (300, 0.4, 5)])
def test_planted_outliers_are_found(mode, n, frac, seed):
    """0.5 px noise, 25-40 % outliers displaced by 20-60 px, 100 rows: every planted outlier is in the outlier list, the pose is
    near the truth, the reference would return true"""
    rng = np.random.default_rng(seed)
    bv, X, Rw, C, planted = R.make_scene(rng, n, noise_px=0.5, outlier_frac=frac)
    res = R.search(bv, X, R.draw_samples(seed, n, 100), mode, 100, TH)
    assert res["status"] == 0 and res["best_row"] >= 0
    assert set(np.nonzero(planted)[0]) <= set(res["outliers"].tolist())
    assert np.all(np.diff(res["outliers"]) > 0)
    assert res["n_inliers"] + len(res["outliers"]) == n
    assert np.abs(res["model"][:9].reshape(3, 3) - Rw).max() < 0.02 and np.abs(res["model"][9:] - C).max() < 0.2


def _scene(seed=7, n=40, **kw):
    rng = np.random.default_rng(seed)
    bv, X, _, _, _ = R.make_scene(rng, n, **kw)
    return bv, X


@pytest.mark.parametrize("mode", [R.LMEDS, R.RANSAC], ids=["lmeds", "ransac"])
def test_a_skipped_row_does_not_count(mode):
    bv, X = _scene(noise_px=0.5, outlier_frac=0.3)
    good = R.dedup_rows(R.draw_samples(1, 40, 6))
    table = np.concatenate([[[3, 3, 5, 6]], good[:1], [[1, 2, 40, 4]], good[1:]]).astype(np.int32)
    res = R.search(bv, X, table, mode, 2, TH)
    assert list(res["trace_valid"][:3]) == [0, 1, 0]
    if mode == R.LMEDS:
        assert res["iterations"] == 2 and res["rows_consumed"] == 4      # two invalid rows passed on the way to two counted ones
    else:
        assert res["iterations"] == 3 and res["rows_consumed"] == 5      # RANSAC breaks once iterations > max_iterations
    assert res["best_row"] not in (0, 2)


@pytest.mark.parametrize("mode", [R.LMEDS, R.RANSAC], ids=["lmeds", "ransac"])
def test_ties_keep_the_first(mode):
    bv, X = _scene(noise_px=0.5, outlier_frac=0.3)
    row = R.draw_samples(2, 40, 1)
    res = R.search(bv, X, np.concatenate([row, row, row]), mode, 3, TH)
    assert res["trace_score"][0] == res["trace_score"][1] == res["trace_score"][2] and res["best_row"] == 0


def test_ransac_stops_early_on_a_clean_scene():
    """all points inliers: w = 1, q clamps to DBL_EPSILON, k = log(0.01) / log(eps) = 0.13 < 1: one iteration"""
    bv, X = _scene()
    res = R.search(bv, X, R.draw_samples(3, 40, 50), R.RANSAC, 100, TH)
    assert res["iterations"] == 1 and res["rows_consumed"] == 1 and res["score"] == 40 and res["status"] == 0
    assert len(res["outliers"]) == 0
    lm = R.search(bv, X, R.draw_samples(3, 40, 50), R.LMEDS, 100, TH)
    assert lm["iterations"] == 50 and lm["rows_consumed"] == 50      # LMedS has no early exit: the rows run out


def test_fewer_than_four_points():
    bv, X = _scene(n=3)
    res = R.search(bv, X, np.zeros((0, 4), np.int32), R.LMEDS, 100, TH)
    assert res["status"] == R.TOO_FEW_POINTS and res["best_row"] == -1 and res["iterations"] == 0 and len(res["outliers"]) == 0
    res = R.search(np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 4), np.int32), R.RANSAC, 100, TH)
    assert res["status"] == R.TOO_FEW_POINTS


def test_no_valid_row_and_fewer_than_five_inliers():
    bv, X = _scene()
    res = R.search(bv, X, np.array([[0, 0, 1, 2], [5, 6, 7, 99]], np.int32), R.LMEDS, 100, TH)
    assert res["status"] == (R.NO_MODEL | R.FEW_INLIERS) and res["rows_consumed"] == 2 and res["iterations"] == 0
    rng = np.random.default_rng(11)            # bearings that have nothing to do with the points
    n = 12
    bv = rng.normal(size=(n, 3)) + [0, 0, 3]
    bv /= np.linalg.norm(bv, axis=1)[:, None]
    X = rng.uniform(-3, 3, (n, 3))
    for mode in (R.LMEDS, R.RANSAC):
        res = R.search(bv, X, R.draw_samples(4, n, 30), mode, 30, TH)
        assert res["best_row"] >= 0 and res["n_inliers"] < 5 and res["status"] & R.FEW_INLIERS and not res["status"] & R.NO_MODEL


def test_even_and_odd_median():
    assert R.penalty(np.array([4.0, 1.0, 9.0, 16.0])) == 2.5 and R.penalty(np.array([4.0, 1.0, 9.0])) == 2.0
    for n in (10, 11):
        bv, X = _scene(n=n, noise_px=0.5)
        row = R.draw_samples(5, n, 1)
        res = R.search(bv, X, row, R.LMEDS, 1, TH)
        m = R.hypothesis(row[0], bv, X)
        s = np.sqrt(np.sort(R.distances(m[:, :3], m[:, 3], bv, X)))
        want = s[n // 2] if n % 2 else (s[n // 2 - 1] + s[n // 2]) / 2
        assert res["score"] == want and res["best_row"] == 0


def test_clamp_keeps_the_square_root_real():
    """a sample point's own 1 - cos comes out slightly negative about half of the time: clamped to 0, never NaN"""
    rng = np.random.default_rng(13)
    negatives = 0
    for _ in range(50):
        bv, X, _, _, _ = R.make_scene(rng, 9)
        m = R.hypothesis([0, 1, 2, 3], bv, X)
        v = (X[:3] - m[:, 3]) @ m[:, :3]
        raw = 1 - (bv[:3] * (v / np.linalg.norm(v, axis=1)[:, None])).sum(axis=1)
        negatives += int((raw < 0).sum())
        d = R.distances(m[:, :3], m[:, 3], bv, X)
        assert (d >= 0).all() and np.isfinite(np.sqrt(d)).all() and np.isfinite(R.penalty(d))
    assert negatives > 0
    nan = R.distances(np.eye(3), np.zeros(3), np.array([[0, 0, 1.0]]), np.zeros((1, 3)))      # X == C: 0 / 0
    assert nan[0] == 0


KNOWN = {(1, 9, 3): [[5, 7, 3, 2], [3, 5, 0, 1], [6, 7, 2, 1]], (2, 300, 2): [[10, 26, 51, 36], [49, 219, 62, 155]]}


def test_generator_known_answers():
    assert R._splitmix64(0, 0) == 0xE220A8397B1DCDAF          # splitmix64's first output for the state 0
    for (seed, n, rows), want in KNOWN.items():
        got = R.draw_samples(seed, n, rows)
        assert got.dtype == np.int32 and got.tolist() == want
    t = R.draw_samples(99, 5, 200)
    assert all(len(set(r)) == 4 for r in t.tolist()) and t.min() == 0 and t.max() == 4


def test_library_generator_gives_the_same_integers():
    from ov2slam_amd import pose
    from ov2slam_amd import _lib as L
    for (seed, n, rows), want in KNOWN.items():
        assert pose.draw_samples(seed, n, rows).tolist() == want
    for seed, n, rows in ((0, 4, 50), (2 ** 63 + 5, 2048, 300), (12345, 17, 0)):
        assert np.array_equal(pose.draw_samples(seed, n, rows), R.draw_samples(seed, n, rows))
    with pytest.raises(L.Ov2Error):
        pose.draw_samples(1, 3, 1)
