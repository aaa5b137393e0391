"""The specification of the local-map matching (tests/match_ref.py) against itself: the literal replay of the reference loop
(Mapper::matchToMap, src/mapper.cpp:576-774) and the flattened per-map-point form that k_map_match<false> implements agree bit for bit on
randomised scenes that make the interesting paths common, the crafted quirks behave as the header says, and the forward
distortion model agrees with the published model evaluated in extended precision.  No GPU."""
import copy
import math

import numpy as np
import pytest

from tests import match_ref as R

CALIBS = {
    "nodist": dict(D=None, model="pinhole"),
    "radtan4": dict(D=R.RADTAN4, model="pinhole"),
    "radtan5": dict(D=R.RADTAN5, model="pinhole"),
    "fisheye": dict(D=R.FISHEYE4, model="fisheye"),
}
SEEDS = (0, 1, 2)
_campaign = {}


def _run(calib, nb3d, seed):
    key = (calib, nb3d, seed)
    if key not in _campaign:
        P = R.make_params(**CALIBS[calib])
        M = R.make_scene(P, np.random.default_rng(seed * 100 + nb3d + len(calib)), nb3dkps=nb3d, n_kp=90, n_lm=200)
        kf, meta = R.flatten(M)
        ev = {}
        rep = R.replay_arrays(M, meta, ev=ev)
        _campaign[key] = (M, kf, meta, rep, ev)
    return _campaign[key]


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("nb3d", [20, 100])
@pytest.mark.parametrize("calib", list(CALIBS))
def test_replay_equals_flat(calib, nb3d, seed):
    M, kf, meta, rep, _ = _run(calib, nb3d, seed)
    got = R.flat(M["params"], kf)
    ok, field = R.same(got, rep)
    assert ok, field
    assert not any(int(v) == -1 for v in kf["obs_kf"]), "the campaign holds no stale observation: replay and flat agree exactly"
    # map_previd_newid itself, keyed by the ids
    prev_new, _ = R.replay(copy.deepcopy(M))
    mine = {meta["kp_lmid"][k]: meta["lm_lmid"][l] for k, l in enumerate(got["kp_lm"]) if l >= 0}
    assert mine == prev_new


def test_campaign_reaches_every_path():
    """conditions on the generated inputs, judged on the replay of the reference loop alone"""
    bits, ev, planted, matched = 0, {}, 0, 0
    for calib in CALIBS:
        for nb3d in (20, 100):
            for seed in SEEDS:
                M, kf, meta, rep, e = _run(calib, nb3d, seed)
                for s in rep["lm_status"]:
                    bits |= int(s)
                for k, v in e.items():
                    if k != "margin":
                        ev[k] = ev.get(k, 0) + v
                lm_row = {i: r for r, i in enumerate(meta["lm_lmid"])}
                kp_row = {i: r for r, i in enumerate(meta["kp_lmid"])}
                for a, b in M["planted"]:
                    planted += 1
                    matched += int(rep["kp_lm"][kp_row[b]] == lm_row[a])
    assert bits == 63, bits
    for gate in ("gate_pxdist", "gate_shared", "gate_coproj", "tie_best", "tie_pick"):
        assert ev.get(gate, 0) >= 1, (gate, ev)
    assert planted >= 100 and matched >= planted / 4, (planted, matched)


@pytest.mark.parametrize("case", R.crafted_cases(), ids=lambda c: c[0])
def test_crafted_quirks(case):
    name, M, status, lm_kp = case
    kf, meta = R.flatten(M)
    got = R.flat(M["params"], kf)
    assert [int(s) for s in got["lm_status"]] == status
    assert [int(k) for k in got["lm_kp"]] == lm_kp
    snap = R.replay_arrays(M, meta, mutate=False)
    ok, field = R.same(got, snap)
    assert ok, field
    lit = R.replay_arrays(M, meta, mutate=True)
    if name == "stale_observation_snapshot":
        # the reference cleans B's observer set while it handles the first point, so its second point is no longer barred
        assert int(lit["lm_status"][1]) == R.BEST and int(got["lm_status"][1]) == R.NO_CANDIDATE
        assert int(kf["obs_kf"][kf["obs_start"][kf["kp_mp"][0]] + 1]) == -1
    else:
        ok, field = R.same(got, lit)
        assert ok, field


def test_more_than_64_observers_sum_order_matters():
    """the crafted 80-observer row: summing the same distances in descending order gives another float, so the case does pin the
    order of the sum"""
    name, M, _, _ = [c for c in R.crafted_cases() if c[0] == "more_than_64_observers"][0]
    P = M["params"]
    w = tuple(R.D(v) for v in M["mps"][10]["wpt"])
    d = [R.pt_dist(M["kfs"][k]["mapkps_"][1], R.project_dist(P, R.se3_act(R.pose(M["kfs"][k]["Tcw"]), w))) for k in sorted(M["kfs"])]
    assert len(d) == 80

    def fsum(seq):
        acc = R.F32(0)
        for v in seq:
            acc = R.F32(R.D(acc) + v)
        return acc
    assert fsum(d) != fsum(d[::-1])


# ---- the forward distortion model -------------------------------------------------------------------------------------------------------
def _published(P, x, y):
    """the published models in extended precision on the float-rounded normalised point"""
    L = np.longdouble
    fx, fy, cx, cy = (L(v) for v in P["K"])
    k = [L(v) for v in P["D"]] + [L(0)] * (12 - len(P["D"]))
    x, y = L(x), L(y)
    if P["model"] == "fisheye":
        r = np.sqrt(x * x + y * y)
        th = L(math.atan(float(r)))
        thd = th * (1 + k[0] * th ** 2 + k[1] * th ** 4 + k[2] * th ** 6 + k[3] * th ** 8)
        s = thd / r if r > 1e-8 else L(1)
        return x * s * fx + cx, y * s * fy + cy
    k1, k2, p1, p2, k3, k4, k5, k6, s1, s2, s3, s4 = k
    r2 = x * x + y * y
    rad = (1 + k1 * r2 + k2 * r2 ** 2 + k3 * r2 ** 3) / (1 + k4 * r2 + k5 * r2 ** 2 + k6 * r2 ** 3)
    xd = x * rad + 2 * p1 * x * y + p2 * (r2 + 2 * x * x) + s1 * r2 + s2 * r2 ** 2
    yd = y * rad + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y + s3 * r2 + s4 * r2 ** 2
    return xd * fx + cx, yd * fy + cy


RATIONAL8 = R.RADTAN5 + (0.012, -0.004, 0.0007)
PRISM12 = RATIONAL8 + (0.0004, -0.0002, 0.0003, 0.0001)


@pytest.mark.parametrize("name,D,model", [("radtan4", R.RADTAN4, "pinhole"), ("radtan5", R.RADTAN5, "pinhole"),
                                          ("rational8", RATIONAL8, "pinhole"), ("prism12", PRISM12, "pinhole"),
                                          ("fisheye4", R.FISHEYE4, "fisheye")])
def test_forward_distortion_within_one_float_ulp(name, D, model):
    P = R.make_params(D=D, model=model)
    rng = np.random.default_rng(5)
    worst = 0.0
    for _ in range(2000):
        z = rng.uniform(0.3, 20)
        p = (rng.uniform(-0.9, 0.9) * z, rng.uniform(-0.6, 0.6) * z, z)
        u, v = R.project_dist(P, p)
        invz = R.D(1) / R.D(p[2])
        x, y = R.F32(R.D(p[0]) * invz), R.F32(R.D(p[1]) * invz)
        eu, ev = _published(P, x, y)
        for got, want in ((u, eu), (v, ev)):
            ulp = float(np.spacing(np.float32(abs(float(want)))))
            worst = max(worst, abs(float(np.longdouble(got) - want)) / ulp)
    assert worst <= 1.0, worst


def test_no_coefficients_is_the_plain_pinhole_bit_for_bit():
    P = R.make_params()
    fx, fy, cx, cy = (R.D(v) for v in P["K"])
    rng = np.random.default_rng(6)
    for _ in range(500):
        p = tuple(R.D(v) for v in (rng.normal(0, 3), rng.normal(0, 3), rng.uniform(0.1, 20)))
        invz = R.D(1) / p[2]
        want = (R.F32(fx * (p[0] * invz) + cx), R.F32(fy * (p[1] * invz) + cy))
        got = R.project_dist(P, p)
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
    assert R.project_dist(dict(P, D=()), (1.0, 2.0, 4.0)) == R.project_dist(P, (1.0, 2.0, 4.0))
