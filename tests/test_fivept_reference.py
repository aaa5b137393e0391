"""The specification of the 5-point search (tests/fivept_ref.py) against ground truth, without a GPU: the solver recovers a known
relative pose, every candidate it returns is an essential matrix through its five matches, the Sturm root count is numpy's, Horn's
closed form is the SVD decomposition, and the loop obeys each of its rules.  np.linalg is used HERE, as the independent yardstick;
the specification itself does without."""
import math

import numpy as np
import pytest

from tests import fivept_ref as R

TH = R.threshold_of(3.0, 460.0, 460.0)
N_SCENES = 200
_cache = {}


def scenes():
    """200 noise-free eight-point scenes, each solved in float64 and in longdouble"""
    if "s" not in _cache:
        out = []
        for s in range(N_SCENES):
            bv1, bv2, Rt, tt, _ = R.make_scene(np.random.default_rng(s), 8)
            row = list(range(8))
            out.append(dict(bv1=bv1, bv2=bv2, R=Rt, t=tt, hyp=R.hypothesis(row, bv1, bv2), five=R.solve_five(bv1[:5], bv2[:5]),
                            five_ld=R.solve_five(bv1[:5].astype(np.longdouble), bv2[:5].astype(np.longdouble), np.longdouble)))
        _cache["s"] = out
    return _cache["s"]


def test_noise_free_scenes_give_the_true_pose():
    worst = 0.0
    for c in scenes():
        m, n_roots, pick = c["hyp"]
        assert m is not None and n_roots >= 1 and pick[0] >= 0
        worst = max(worst, float(np.abs(m[:, :3] - c["R"]).max()), float(np.abs(m[:, 3] - c["t"]).max()))
    print("worst |model - truth| over %d scenes: %.3g" % (N_SCENES, worst))
    # MEASURED 3.4e-06 over these 200 scenes (5.8e-07 over the first 40) (the conditioning of the degree-10 polynomial sets it: the same code in longdouble
    # reaches 1e-10 on the worst scene); the bound is 100 x that
    assert worst <= 3.4e-4


def _residuals(E, f1, f2):
    E = np.asarray(E, np.float64).reshape(3, 3)
    E = E / np.sqrt((E * E).sum())
    cubic = 2 * E @ E.T @ E - np.trace(E @ E.T) * E
    epi = np.array([f1[i] @ E @ f2[i] for i in range(5)])
    return abs(np.linalg.det(E)), np.abs(cubic).max(), np.abs(epi).max()


def test_every_candidate_is_an_essential_matrix_through_its_five_matches():
    """For E of unit Frobenius norm the three residuals are polynomials in E's entries with gradients of order 1 to 10, so an E
    that is off by e leaves residuals of at most ~10 e.  e is measured per candidate as the distance to the same candidate of the
    longdouble run (unit norm, same sign); the allowance is 100 x that plus 1e-12 for the roundings of the residuals themselves.
    The five epipolar equations do not depend on the root at all (E lies in the null space by construction): 1e-12 alone."""
    checked = 0
    for c in scenes():
        (Es, info), (El, infol) = c["five"], c["five_ld"]
        assert len(Es) >= 1
        if len(Es) != len(El):
            continue
        for E, Eld in zip(Es, El):
            a, b = E / np.sqrt((E * E).sum()), Eld / np.sqrt((Eld * Eld).sum())
            e = float(np.abs(a - b).max())
            det, cubic, epi = _residuals(E, c["bv1"], c["bv2"])
            assert epi <= 1e-12, epi
            assert det <= 1e-12 + 100 * e and cubic <= 1e-12 + 100 * e, (det, cubic, e)
            checked += 1
    print("candidates checked: %d" % checked)
    assert checked >= 3 * N_SCENES


def test_real_root_count_is_numpys():
    compared = 0
    for c in scenes():
        info = c["five"][1]
        z = np.roots(info["poly"])
        if np.any(np.abs(z.imag[z.imag != 0]) < 1e-6):
            continue                                               # a nearly double root: the count is not defined to rounding
        compared += 1
        real = np.sort(z.real[z.imag == 0])
        assert len(info["roots"]) == len(real)
        assert all(info["roots"][i] <= info["roots"][i + 1] for i in range(len(real) - 1))
        scale = np.maximum(1.0, np.abs(real))
        assert np.all(np.abs(np.array(info["roots"], np.float64) - real) <= 1e-6 * scale)
    print("polynomials compared: %d of %d" % (compared, N_SCENES))
    assert compared >= 0.9 * N_SCENES


def _svd_decomposition(E):
    U, _, Vt = np.linalg.svd(E)
    if np.linalg.det(U) < 0:
        U = -U
    if np.linalg.det(Vt) < 0:
        Vt = -Vt
    W = np.array([[0.0, -1, 0], [1, 0, 0], [0, 0, 1]])
    return [(U @ W @ Vt, U[:, 2]), (U @ W @ Vt, -U[:, 2]), (U @ W.T @ Vt, U[:, 2]), (U @ W.T @ Vt, -U[:, 2])]


def test_horn_is_the_svd_decomposition():
    """on exact essential matrices E = s [t]x R: the four (R, t) of Horn's closed form are the four of the SVD, as sets, to 1e-12
    (both are a few dozen operations on entries of order 1), and one of them is the (R, t) that made E"""
    rng = np.random.default_rng(3)
    for k in range(100):
        Rt = R._rot(rng, rng.uniform(0.0, 3.0))
        t = rng.normal(size=3)
        t /= np.linalg.norm(t)
        E = rng.uniform(0.1, 10) * rng.choice([-1, 1]) * np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]]) @ Rt
        mine, ref = R.horn(E.reshape(9)), _svd_decomposition(E)
        for Rm, tm in mine:
            assert abs(np.linalg.det(Rm) - 1) < 1e-12 and np.abs(Rm @ Rm.T - np.eye(3)).max() < 1e-12
            assert min(max(np.abs(Rm - Rr).max(), np.abs(tm - tr).max()) for Rr, tr in ref) < 1e-12
        for Rr, tr in ref:
            assert min(max(np.abs(Rm - Rr).max(), np.abs(tm - tr).max()) for Rm, tm in mine) < 1e-12
        assert min(max(np.abs(Rm - Rt).max(), np.abs(tm - t).max()) for Rm, tm in mine) < 1e-12
        assert np.array_equal(mine[0][1], mine[1][1]) and np.array_equal(mine[2][1], -mine[0][1])


def test_threshold_known_answer():
    # tan(a) = q, the float quotient 3 / 460: cos(a) = 1 / sqrt(1 + q^2), and 1 - cos(a) = q^2 / (s (1 + s)) with s = sqrt(1 + q^2)
    q = float(np.float32(3.0) / np.float32(460.0))
    s = math.sqrt(1.0 + q * q)
    want = 2.0 * q * q / (s * (1.0 + s))
    assert abs(R.threshold_of(3.0, 460.0, 460.0) - want) <= 1e-10 * want       # 1 - cos cancels five of sixteen digits
    assert abs(want - 2.0 * (1.0 - 460.0 / math.sqrt(460.0 ** 2 + 9.0))) <= 1e-6 * want      # and 3 / 460 is 3 / 460
    # the focal length is the FLOAT (fx + fy) / 2 and the quotient a float (src/multi_view_geometry.cpp:654-658)
    f = np.float32(np.float32(458.654) + np.float32(457.296)) / np.float32(2)
    q = float(np.float32(3.0) / f)
    assert R.threshold_of(3.0, 458.654, 457.296) == 2.0 * (1.0 - math.cos(math.atan(q)))
    assert 0.9 < R.threshold_of(3.0, 458.654, 457.296) / (2.0 * (1.0 - math.cos(math.atan(3.0 / 457.975)))) < 1.1


def _fake(counts, n=100):
    """prepared rows whose inlier counts are given (None: an invalid row): the loop reads nothing else"""
    models, dist = [], []
    for c in counts:
        if c is None:
            models.append(None); dist.append(None)
        else:
            models.append(np.concatenate([np.eye(3), [[1.0], [0], [0]]], axis=1) + len(models))      # the row's number marks its model
            dist.append(np.where(np.arange(n) < c, 0.0, 1.0))
    z = np.tile([0, 0, 1.0], (n, 1))
    sm = np.tile(np.arange(8, dtype=np.int32), (len(counts), 1))
    return z, z, sm, (models, dist, [1] * len(counts), [(0, 0)] * len(counts))


def _loop(counts, max_iterations=1000, n=100):
    bv1, bv2, sm, prep = _fake(counts, n)
    return R.search(bv1, bv2, sm, max_iterations, 0.5, prep=prep)


def test_loop_skipped_rows_do_not_count():
    r = _loop([None, None, 50, None, 50])
    assert r["iterations"] == 2 and r["rows_consumed"] == 5 and r["best_row"] == 2 and list(r["trace_valid"]) == [0, 0, 1, 0, 1]
    r = _loop([None, None])
    assert r["status"] == R.NO_MODEL | R.FEW_INLIERS and r["best_row"] == -1 and r["iterations"] == 0 and r["rows_consumed"] == 2
    assert not r["model"].any() and len(r["outliers"]) == 0


def test_loop_a_tie_keeps_the_first():
    r = _loop([40, 60, 60, 50, 60])
    assert r["best_row"] == 1 and r["score"] == 60 and r["model"][0] == 2.0          # eye + row number 1
    assert np.array_equal(r["outliers"], np.arange(60, 100, dtype=np.int32)) and r["n_inliers"] == 60


def test_loop_adaptive_bound_with_a_sample_of_eight():
    # 90 of 100: k = log(0.01) / log(1 - 0.9^8) = 8.18: the loop runs nine iterations
    k = math.log(0.01) / math.log(1 - 0.9 ** 8)
    assert 8 < k < 9
    r = _loop([90] * 20)
    assert r["iterations"] == 9 and r["rows_consumed"] == 9 and r["best_row"] == 0
    # every point an inlier: 1 - w^8 is clamped to DBL_EPSILON, k = log(0.01) / log(eps) < 1: one iteration
    r = _loop([100] * 20)
    assert r["iterations"] == 1 and r["rows_consumed"] == 1
    # a better row late shortens the search: 50 gives k = 1177, then 95 gives k = log(0.01) / log(1 - 0.95^8) = 4.2 < 5 iterations done
    r = _loop([50, 50, 50, 50, 95, 50, 50])
    assert r["iterations"] == 5 and r["best_row"] == 4
    # with a sample of 4 the first case would stop after log(0.01) / log(1 - 0.9^4) = 4.3 -> 5 iterations
    assert math.log(0.01) / math.log(1 - 0.9 ** 4) < 5
    # the bound on the iterations is checked after the increment: max_iterations + 1 rows count
    r = _loop([50] * 20, max_iterations=3)
    assert r["iterations"] == 4 and r["rows_consumed"] == 4
    r = _loop([50] * 3, max_iterations=1000)
    assert r["iterations"] == 3 and r["rows_consumed"] == 3                     # the table runs out


def test_loop_fewer_than_ten_inliers():
    assert _loop([9, 5])["status"] == R.FEW_INLIERS and _loop([9, 5])["best_row"] == 0
    assert _loop([10, 5])["status"] == 0
    bv1, bv2, sm, prep = _fake([5], n=7)
    assert R.search(bv1, bv2, sm, 10, 0.5, prep=prep)["status"] == R.TOO_FEW_POINTS


def test_invalid_rows():
    bv1, bv2, _, _, _ = R.make_scene(np.random.default_rng(1), 20)
    for row in ([0, 1, 2, 3, 4, 5, 6, 6], [0, 1, 2, 3, 4, 5, 6, 20], [-1, 1, 2, 3, 4, 5, 6, 7]):
        assert R.hypothesis(row, bv1, bv2)[0] is None
    assert R.hypothesis([0, 1, 2, 3, 4, 5, 6, 7], bv1, bv2)[0] is not None
    with np.errstate(all="ignore"):
        m = R.hypothesis([0, 1, 2, 3, 4, 5, 6, 7], bv1, bv1)[0]     # zero parallax: whatever comes out is finite or nothing
    assert m is None or np.all(np.isfinite(m))


def test_planted_outliers_are_found():
    """30 of 100 matches displaced by 20 - 60 px ACROSS their epipolar lines (a displacement along the line leaves the match
    consistent with the essential matrix: no test on E can see it), 0.5 px of noise, threshold 3 px"""
    bv1, bv2, Rt, tt, planted = R.make_scene(np.random.default_rng(7), 100, noise_px=0.5, outlier_frac=0.3)
    assert planted.sum() == 30
    r = R.search(bv1, bv2, R.draw_samples(7, 100, 60), 60, TH)
    assert r["status"] == 0 and set(np.nonzero(planted)[0]) <= set(r["outliers"].tolist())
    assert r["n_inliers"] >= 0.9 * 70
    assert list(r["outliers"]) == sorted(r["outliers"]) and r["n_inliers"] + len(r["outliers"]) == 100
    # and the true model calls exactly... at least every planted one an outlier and nearly every other match an inlier
    d = R.distances(Rt, tt, bv1, bv2)
    assert np.all(d[planted] >= TH) and (d[~planted] < TH).mean() > 0.95


def test_draw_samples_matches_the_library():
    from ov2slam_amd import pose
    for seed, n, rows in ((1, 8, 5), (77, 130, 200), (2 ** 63 + 5, 9, 33), (0, 2048, 10)):
        a, b = pose.epipolar_draw_samples(seed, n, rows), R.draw_samples(seed, n, rows)
        assert a.dtype == np.int32 and a.shape == (rows, 8) and np.array_equal(a, b)
        assert all(len(set(r.tolist())) == 8 and r.min() >= 0 and r.max() < n for r in b)
    with pytest.raises(ValueError):
        R.draw_samples(1, 7, 1)
    # the first draws are those of the P3P stream: one stream, wider rows
    from tests import p3p_ref
    assert list(R.draw_samples(5, 1000, 1)[0][:4]) == list(p3p_ref.draw_samples(5, 1000, 1)[0])
