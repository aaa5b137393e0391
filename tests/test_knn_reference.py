"""The numpy specification of the loop closer's descriptor matching (tests/knn_ref.py): the transcription of the OpenCV path
(replay) and the order-free statement (flat) agree on every field over a generated campaign and all crafted cases, the campaign
reaches every branch it is meant to, the crafted literals hold, and the 0.85 ratio test in fp64 (and in float32) is the exact
20 d0 <= 17 d1 over the whole range of distances."""
import numpy as np
import pytest

from tests import knn_ref as R

SIZES = [(1, 1), (1, 2), (3, 1), (7, 3), (40, 17), (64, 64), (65, 63), (33, 120), (120, 33), (90, 257), (150, 150), (257, 40)]
# train sets of two and three rows whose planted row sits at max_dist or max_dist + 1: with so few rows the nearest one is often
# beyond the distance gate, which a larger random train set never shows (its nearest row is around 105)
GATE_SIZES = [(20, 2), (20, 3)]


def _campaign():
    ev, n = {}, 0
    for seed in range(2):
        for n_q, n_t in SIZES + GATE_SIZES:
            rng = np.random.default_rng(1000 * seed + 7 * n_q + n_t)
            q, t = R.make_case(rng, n_q, n_t, **(dict(true_frac=0.0, gate_frac=1.0) if (n_q, n_t) in GATE_SIZES else {}))
            a, b = R.replay(q, t, ev=ev), R.flat(q, t)
            ok, field = R.same(a, b)
            assert ok, (seed, n_q, n_t, field)
            assert len(a["pairs"]) == int(a["good"].sum())
            n += 1
    return ev, n


def test_replay_equals_flat_on_generated_cases_and_reaches_every_branch():
    ev, n = _campaign()
    assert n >= 24
    # the generated cases alone meet both kinds of good and of rejected rows and both ties
    for key in ("good_ratio", "good_single", "rej_dist", "rej_ratio", "tie_first", "tie_second"):
        assert ev.get(key, 0) > 0, (key, ev)
    for name, q, t, D, Rt, good, idx in R.crafted_cases():
        R.replay(q, t, D, Rt, ev=ev)
    assert ev.get("ratio_equality", 0) >= len(R.RATIO_EQUALITIES), ev


@pytest.mark.parametrize("case", R.crafted_cases(), ids=lambda c: c[0])
def test_crafted_cases(case):
    name, q, t, D, Rt, good, idx = case
    a, b = R.replay(q, t, D, Rt), R.flat(q, t, D, Rt)
    ok, field = R.same(a, b)
    assert ok, (name, field)
    assert [int(g) for g in b["good"]] == good
    assert [[int(v) for v in row] for row in b["idx"]] == idx
    assert [[int(u), int(v)] for u, v in b["pairs"]] ==[[i, idx[i][0]] for i, g in enumerate(good) if g]


def test_non_default_parameters_agree():
    rng = np.random.default_rng(5)
    q, t = R.make_case(rng, 80, 90)
    for D, Rt in ((96, 0.7), (256, 1.0), (0, 0.0), (20, 0.85)):
        ok, field = R.same(R.replay(q, t, D, Rt), R.flat(q, t, D, Rt))
        assert ok, (D, Rt, field)
    assert R.flat(q, t, 256, 1.0)["good"].all()                        # d0 <= d1 always holds


def test_quirks():
    rng = np.random.default_rng(9)
    q = rng.integers(0, 256, (5, 32), dtype=np.uint8)
    one = (~q[:1]).astype(np.uint8)                                     # at distance 256 from query row 0
    r = R.flat(q, one)
    assert r["good"].all() and r["dist"][0, 0] == 256 and (r["idx"][:, 1] == -1).all() and (r["dist"][:, 1] == -1).all()
    assert len(R.flat(q[:0], one)["pairs"]) == 0 and len(R.flat(q, one[:0])["pairs"]) == 0
    assert not R.flat(q, one[:0])["good"].any()
    same_row = np.stack([q[2], q[2]])
    r = R.flat(q[2:3], same_row)
    assert r["dist"].tolist() == [[0, 0]] and r["idx"].tolist() == [[0, 1]] and r["good"].tolist() == [1]
    assert R.MAX_DIST == 128 == int(32 * 0.5 * 8.)


def test_ratio_085_in_fp64_is_the_exact_integer_test():
    """(double)d0 <= (double)d1 * 0.85 against 20 d0 <= 17 d1 for all 0 <= d0 <= d1 <= 256; the float32 product decides alike"""
    eq = []
    for d1 in range(257):
        for d0 in range(d1 + 1):
            exact = 20 * d0 <= 17 * d1
            assert R.ratio_ok(d0, d1, 0.85) == exact, (d0, d1)
            assert bool(np.float32(d0) <= np.float32(np.float32(d1) * np.float32(0.85))) == exact, (d0, d1)
            if 20 * d0 == 17 * d1 and d0 > 0:
                eq.append((d0, d1))
    assert eq == [(17 * m, 20 * m) for m in range(1, 13)] and eq[-1] == (204, 240)
    assert all(R.ratio_ok(a, b, 0.85) for a, b in eq)
    assert R.RATIO_EQUALITIES == [e for e in eq if e[0] <= 128]
    assert R.ratio_ok(0, 0, 0.85)
