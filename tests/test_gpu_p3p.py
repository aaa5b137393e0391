"""The device P3P pose search (csrc/p3p.hip, ov2_p3p_ransac[_batch]) against the numpy specification (tests/p3p_ref.py).
Decisions are compared exactly (outlier list, status, iterations, rows consumed, valid flags, the best row wherever the
specification's own margins say the choice is not a near-tie), numbers at a tolerance.

TOLERANCE.  The specification run in float64 and the same code in np.longdouble, over the committed cases below (both modes,
measure_float64_error() at the bottom of this file prints the figures):
    best model and its score, largest absolute difference        MEASURED_BEST  = 2.22e-12
    every valid row's LMedS penalty, largest absolute difference MEASURED_TRACE = 2.29e-10  (set by the worst-conditioned of some 10^4 rows)
The device may differ from numpy by more than one rounding (another quartic solver, other sqrt / division sequences), so 100 x
that is allowed: TOL_BEST = 2.22e-10 on the model (entries of order 1 to 10) and on the score, TOL_TRACE = 2.29e-8 on the per-row
penalties.  Inlier counts are integers and are compared exactly."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import p3p_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEASURED_BEST, MEASURED_TRACE = 2.22e-12, 2.29e-10
TOL_BEST, TOL_TRACE = 100 * MEASURED_BEST, 100 * MEASURED_TRACE
TH = R.threshold_of(3.0, 460.0, 460.0)
NS = (9, 16, 63, 64, 65, 130, 300, 513)        # 513: one past the 512 points whose distances stay in registers
SS = (1, 100, 1000)
MODES = {"lmeds": R.LMEDS, "ransac": R.RANSAC}
MARGIN = 1e-6

_cache = {}


def scene(n, S):
    """the committed case (n, S): 0.5 px noise, 30 % outliers, the table of seed 1000 n + S without repeated triples, and the
    specification's evaluation of every row (shared by both modes)"""
    key = (n, S)
    if key not in _cache:
        rng = np.random.default_rng(100000 + 1000 * n + S)
        bv, X, Rw, C, planted = R.make_scene(rng, n, noise_px=0.5, outlier_frac=0.3)
        sm = R.dedup_rows(R.draw_samples(1000 * n + S, n, S))
        _cache[key] = dict(bv=bv, X=X, samples=sm, prep=R.prepare(bv, X, sm), Rw=Rw, C=C)
    return _cache[key]


def spec(n, S, mode):
    key = (n, S, mode)
    if key not in _cache:
        c = scene(n, S)
        _cache[key] = R.search(c["bv"], c["X"], c["samples"], mode, len(c["samples"]), TH, prep=c["prep"])
    return _cache[key]


def clear_of_ties(res):
    return res["gap"] >= MARGIN and res["th_margin"] >= MARGIN


def test_margins_of_the_committed_cases():
    """no GPU: at least 90 % of the committed cases clear both margins, so that the best row is compared exactly there"""
    flags = [clear_of_ties(spec(n, S, m)) for n in NS for S in SS for m in MODES.values() if S > 1]
    print("cases clear of near-ties: %d of %d" % (sum(flags), len(flags)))
    assert sum(flags) >= 0.9 * len(flags)


def _outliers_of(c, row):
    return np.nonzero(~(c["prep"][1][row] < TH))[0].astype(np.int32)


def _compare(c, want, got, mode):
    assert got["status"] == want["status"]
    assert got["iterations"] == want["iterations"] and got["rows_consumed"] == want["rows_consumed"]
    assert np.array_equal(got["trace_valid"], want["trace_valid"])
    if mode == R.RANSAC:
        assert np.array_equal(got["trace_score"], want["trace_score"])
    else:
        worst = np.abs(got["trace_score"] - want["trace_score"]).max() if len(want["trace_score"]) else 0.0
        at = int(np.abs(got["trace_score"] - want["trace_score"]).argmax()) if len(want["trace_score"]) else -1
        print("largest per-row penalty difference %.3g in row %d (allowed %.3g)" % (worst, at, TOL_TRACE))
        assert worst <= TOL_TRACE
    row = got["best_row"]
    if row != want["best_row"]:
        # only a near-tie may be decided the other way: then the device's row must be the other side of that tie
        assert not clear_of_ties(want), "best row %d, specification %d, margins %g / %g" % (row, want["best_row"], want["gap"], want["th_margin"])
        assert row >= 0 and want["trace_valid"][row]
        assert abs(want["trace_score"][row] - want["score"]) <= MARGIN * abs(want["score"])
    if row < 0:
        assert len(got["outliers"]) == 0 and not got["model"].any()
        return
    m = c["prep"][0][row]
    model = np.concatenate([m[:, :3].reshape(9), m[:, 3]])
    dm, ds = np.abs(got["model"] - model).max(), abs(got["score"] - want["trace_score"][row])
    print("model difference %.3g, score difference %.3g (allowed %.3g)" % (dm, ds, TOL_BEST))
    assert dm <= TOL_BEST and ds <= TOL_BEST
    assert got["outliers"].dtype == np.int32 and np.array_equal(got["outliers"], _outliers_of(c, row))
    assert got["n_inliers"] == len(c["bv"]) - len(got["outliers"])


@pytest.mark.gpu
@pytest.mark.parametrize("mode", list(MODES), ids=list(MODES))
@pytest.mark.parametrize("S", SS)
@pytest.mark.parametrize("n", NS)
def test_against_the_specification(gpu_ctx, n, S, mode):
    from ov2slam_amd import pose
    c, want = scene(n, S), spec(n, S, MODES[mode])
    got = pose.p3p_ransac(gpu_ctx, pose.p3p_params(MODES[mode], len(c["samples"]), TH), c, trace=True)
    _compare(c, want, got, MODES[mode])
    if S > 1:
        assert got["ok"] and np.abs(got["Rwc"] - c["Rw"]).max() < 0.05      # and it is the scene's pose


def _mixed_problems(k):
    sizes = [(300, 100), (0, 0), (3, 0), (65, 100), (9, 100), (513, 100), (130, 1000), (16, 1), (64, 100), (63, 1), (3, 0)][:k]
    out = []
    for n, S in sizes:
        if n >= 9:
            c = scene(n, S)
            out.append(dict(bv=c["bv"], X=c["X"], samples=c["samples"]))
        else:
            out.append(dict(bv=np.tile([0, 0, 1.0], (n, 1)), X=np.arange(3.0 * n).reshape(n, 3), samples=np.zeros((0, 4), np.int32)))
    return out


def _same_bytes(a, b):
    for k in ("model", "trace_score"):
        assert np.array_equal(a[k].view(np.uint64), b[k].view(np.uint64)), k
    assert np.array_equal(np.float64(a["score"]).view(np.uint64), np.float64(b["score"]).view(np.uint64))
    for k in ("outliers", "trace_valid"):
        assert np.array_equal(a[k], b[k]), k
    for k in ("best_row", "iterations", "rows_consumed", "status", "n_inliers"):
        assert a[k] == b[k], k


@pytest.mark.gpu
@pytest.mark.parametrize("mode", list(MODES), ids=list(MODES))
@pytest.mark.parametrize("k", [1, 3, 11])
def test_batch_equals_single_calls(gpu_ctx, k, mode):
    """mixed sizes, among them no points and three points: per item the batch form gives the single call's bytes"""
    from ov2slam_amd import pose
    P = pose.p3p_params(MODES[mode], 100, TH)
    pbs = _mixed_problems(k)
    batch = pose.p3p_ransac_batch(gpu_ctx, P, pbs, trace=True)
    assert len(batch) == k
    for pb, b in zip(pbs, batch):
        _same_bytes(pose.p3p_ransac(gpu_ctx, P, pb, trace=True), b)
        if len(pb["bv"]) < 4:
            assert b["status"] == pose.TOO_FEW_POINTS and b["best_row"] == -1 and len(b["outliers"]) == 0 and b["iterations"] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("mode", list(MODES), ids=list(MODES))
def test_two_runs_give_identical_bytes(gpu_ctx, mode):
    from ov2slam_amd import pose
    P = pose.p3p_params(MODES[mode], 1000, TH)
    pbs = _mixed_problems(8)
    a, b = pose.p3p_ransac_batch(gpu_ctx, P, pbs, trace=True), pose.p3p_ransac_batch(gpu_ctx, P, pbs, trace=True)
    for x, y in zip(a, b):
        _same_bytes(x, y)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", list(MODES), ids=list(MODES))
def test_crafted_cases(gpu_ctx, mode):
    from ov2slam_amd import pose
    P = pose.p3p_params(MODES[mode], 50, TH)
    c = scene(65, 100)
    # every row invalid: a repeated index, an index out of range (either side)
    bad = np.array([[1, 1, 2, 3], [0, 1, 2, 65], [-1, 2, 3, 4], [7, 8, 9, 7]], np.int32)
    got = pose.p3p_ransac(gpu_ctx, P, dict(bv=c["bv"], X=c["X"], samples=bad), trace=True)
    want = R.search(c["bv"], c["X"], bad, MODES[mode], 50, TH)
    assert want["status"] == R.NO_MODEL | R.FEW_INLIERS
    _compare(dict(c, prep=R.prepare(c["bv"], c["X"], bad)), want, got, MODES[mode])
    assert got["rows_consumed"] == 4 and got["iterations"] == 0 and not got["trace_valid"].any()
    # collinear world points in the first rows (no plane: the model is not finite), a repeated index, then good rows
    X = c["X"].copy()
    X[1] = X[0] + 0.5 * (X[2] - X[0])
    sm = np.concatenate([[[0, 1, 2, 3], [2, 0, 1, 9], [4, 5, 4, 6]], c["samples"][:20]]).astype(np.int32)
    sm = sm[[i for i, r in enumerate(sm) if i < 3 or not {0, 1, 2} <= set(r[:3].tolist())]]
    got = pose.p3p_ransac(gpu_ctx, P, dict(bv=c["bv"], X=X, samples=sm), trace=True)
    want = R.search(c["bv"], X, sm, MODES[mode], 50, TH)
    assert list(want["trace_valid"][:3]) == [0, 0, 0] and want["trace_valid"][3:].any()
    _compare(dict(c, X=X, prep=R.prepare(c["bv"], X, sm)), want, got, MODES[mode])
    # pure outliers: bearings that have nothing to do with the points
    rng = np.random.default_rng(11)
    n = 12
    bv = rng.normal(size=(n, 3)) + [0, 0, 3]
    bv /= np.linalg.norm(bv, axis=1)[:, None]
    X = rng.uniform(-3, 3, (n, 3))
    sm = R.dedup_rows(R.draw_samples(4, n, 30))
    got = pose.p3p_ransac(gpu_ctx, P, dict(bv=bv, X=X, samples=sm), trace=True)
    want = R.search(bv, X, sm, MODES[mode], 50, TH)
    assert want["status"] & R.FEW_INLIERS and not got["ok"]
    assert got["status"] == want["status"] and np.array_equal(got["trace_valid"], want["trace_valid"])
    if mode == "ransac":          # n < 9: the median is a sample point's rounding noise, only the counts are compared
        _compare(dict(bv=bv, X=X, prep=R.prepare(bv, X, sm)), want, got, MODES[mode])


@pytest.mark.gpu
def test_invalid_arguments_with_a_context(gpu_ctx):
    from ov2slam_amd import pose, _lib as L
    c = scene(16, 1)
    for kw in (dict(threshold=0.0), dict(threshold=float("nan")), dict(boptimize=True), dict(max_iterations=-1)):
        args = dict(mode=R.LMEDS, max_iterations=10, threshold=TH)
        args.update(kw)
        with pytest.raises(L.Ov2Error) as e:
            pose.p3p_ransac(gpu_ctx, pose.p3p_params(**args), c)
        assert e.value.code == L.OV2_EINVAL
    X = c["X"].copy()
    X[3, 1] = np.inf
    with pytest.raises(L.Ov2Error):
        pose.p3p_ransac(gpu_ctx, pose.p3p_params(R.LMEDS, 10, TH), dict(c, X=X))


@pytest.mark.gpu
def test_tracker_bearings_to_p3p_to_pnp(gpu_ctx):
    """the chain VisualFrontEnd::computePose runs: the tracker's bearing vectors of a frame (ov2_tracker_last_keypoints) and their
    world points go through p3p_ransac, its pose through ceresPnP.  Synthetic scene with a known pose; the pose is recovered
    within the bound the specification reaches on the same bearings."""
    import ov2slam_amd
    from ov2slam_amd import pose, synth
    w, h, K = 376, 240, (300.0, 300.0, 188.0, 120.0)
    rng = np.random.default_rng(21)
    n0 = 160
    Rw, C = R._rot(rng, 0.3), rng.uniform(-0.5, 0.5, 3)
    px_true = np.stack([rng.uniform(20, w - 20, n0), rng.uniform(20, h - 20, n0)], axis=1)
    depth = rng.uniform(2.0, 8.0, n0)
    pc = np.stack([(px_true[:, 0] - K[2]) / K[0] * depth, (px_true[:, 1] - K[3]) / K[1] * depth, depth], axis=1)
    X = pc @ Rw.T + C
    planted = np.zeros(n0, bool)
    planted[rng.choice(n0, 40, replace=False)] = True
    X[planted] += rng.uniform(0.5, 1.0, (40, 3))
    px = (px_true + rng.normal(0, 0.3, px_true.shape)).astype(np.float32)      # the observations: 0.3 px of noise
    img = synth.frame_pair(w, h, seed=3)[0]
    vt = ov2slam_amd.VisualFrontEndTracker(gpu_ctx, w, h, use_clahe=False, nbmaxkps=256)
    vt.setCalibration(ov2slam_amd.CameraCalibration(gpu_ctx, "pinhole", *K))
    vt.trackFrame(img, np.zeros((0, 2), np.float32), np.zeros((0, 2), np.float32), None)
    out, st, _ = vt.trackFrame(img, px, px, np.ones(n0, np.uint8))      # the same image: a tracked point stays where it is
    unpx, bv = vt.lastKeypoints(n0)
    vt.close()
    good = (st & 1) > 0
    assert good.sum() >= 80 and np.abs(out[good] - px[good]).max() < 0.05
    unpx, bv, X, planted = np.asarray(unpx, np.float64)[good], np.asarray(bv, np.float64)[good], X[good], planted[good]
    n = len(bv)
    sm = R.dedup_rows(R.draw_samples(5, n, 200))
    want = R.search(bv, X, sm, R.LMEDS, 100, R.threshold_of(3.0, K[0], K[1]))
    got = pose.p3p_ransac(gpu_ctx, pose.p3p_params(pose.LMEDS, 100, pose.threshold(3.0, K[0], K[1])), dict(bv=bv, X=X, samples=sm))
    assert got["ok"] and got["best_row"] == want["best_row"] and np.array_equal(got["outliers"], want["outliers"])
    assert set(np.nonzero(planted)[0]) <= set(got["outliers"].tolist())
    bound = max(np.abs(want["model"][:9].reshape(3, 3) - Rw).max(), np.abs(want["model"][9:] - C).max())
    print("specification's pose error on this scene %.3g" % bound)
    assert np.abs(got["Rwc"] - Rw).max() <= bound + TOL_BEST and np.abs(got["twc"] - C).max() <= bound + TOL_BEST
    # motion-only BA from the P3P pose on its inliers' undistorted pixels
    inl = np.setdiff1d(np.arange(n), got["outliers"])
    q = _quat(got["Rwc"])
    Twc = np.concatenate([got["twc"], q])
    mvg = ov2slam_amd.MultiViewGeometry(gpu_ctx)
    ok, Twc2, out = mvg.ceresPnP(unpx[inl], X[inl], np.zeros(len(inl), np.int32), Twc, 10, 5.9915, True, True, *K)[:3]
    assert ok
    Twc2 = np.asarray(Twc2, np.float64)
    assert np.abs(Twc2[:3] - C).max() <= bound + TOL_BEST and np.abs(_rotm(Twc2[3:]) - Rw).max() <= bound + TOL_BEST


def _quat(Rm):
    """Eigen::Quaterniond(R) for a rotation with positive trace, as [qx qy qz qw]"""
    t = np.trace(Rm)
    assert t > 0
    s = np.sqrt(t + 1.0)
    qw = 0.5 * s
    s = 0.5 / s
    return np.array([(Rm[2, 1] - Rm[1, 2]) * s, (Rm[0, 2] - Rm[2, 0]) * s, (Rm[1, 0] - Rm[0, 1]) * s, qw])


def _rotm(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _wr(f, a):
    a = np.ascontiguousarray(a)
    f.write(struct.pack("<q", a.nbytes)); f.write(a.tobytes())


def _rd(f, dt):
    nb = struct.unpack("<q", f.read(8))[0]
    return np.frombuffer(f.read(nb), dt)


@pytest.mark.gpu
def test_cpp_adapter(gpu_ctx, tmp_path):
    """tests/cpp/p3p_run.cpp: ov2::p3pRansac returns the Python form's pose, outliers and bool, in both modes"""
    from ov2slam_amd import pose
    exe = tmp_path / "p3p_run"
    libdir = os.path.join(ROOT, "ov2slam_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "p3p_run.cpp"),
                           "-o", str(exe), "-L", libdir, "-lov2slam_hip", "-Wl,-rpath," + libdir])
    c = scene(130, 100)
    n, seed, nmaxiter, errth, fx, fy = 130, 77, 100, 3.0, 458.654, 457.296
    case, res = tmp_path / "case.bin", tmp_path / "res.bin"
    with open(case, "wb") as f:
        _wr(f, np.array([nmaxiter, seed], np.int32)); _wr(f, np.array([errth, fx, fy], np.float32)); _wr(f, c["bv"]); _wr(f, c["X"])
    r = subprocess.run([str(exe), str(case), str(res)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    th = pose.threshold(errth, fx, fy)
    with open(res, "rb") as f:
        for use_lmeds in (1, 0):
            ok, Twc, out = _rd(f, np.int32), _rd(f, np.float64), _rd(f, np.int32)
            sm = pose.draw_samples(seed, n, 2 * nmaxiter * (1 if use_lmeds else 10))
            py = pose.p3p_ransac(gpu_ctx, pose.p3p_params(pose.LMEDS if use_lmeds else pose.RANSAC, nmaxiter * (1 if use_lmeds else 10), th),
                                 dict(bv=c["bv"], X=c["X"], samples=sm))
            assert bool(ok[0]) == py["ok"] and py["ok"]
            assert np.array_equal(out, py["outliers"])
            assert np.array_equal(Twc[:3], py["twc"])
            assert np.abs(_rotm(Twc[3:]) - py["Rwc"]).max() <= 1e-14      # a unit quaternion and back: rounding
        small_ok, small_out = _rd(f, np.int32), _rd(f, np.int32)
        assert small_ok[0] == 0 and len(small_out) == 0                  # three points: false, nothing written


def measure_float64_error():
    """prints the figures quoted at the top: float64 against np.longdouble over the committed cases"""
    best = trace = 0.0
    for n in NS:
        for S in SS:
            c = scene(n, S)
            prep_l = R.prepare(c["bv"], c["X"], c["samples"], np.longdouble)
            for mode in MODES.values():
                a = spec(n, S, mode)
                b = R.search(c["bv"], c["X"], c["samples"], mode, len(c["samples"]), TH, F=np.longdouble, prep=prep_l)
                assert np.array_equal(a["trace_valid"], b["trace_valid"])
                if a["best_row"] == b["best_row"]:
                    best = max(best, float(np.abs(a["model"] - b["model"]).max()), float(abs(a["score"] - b["score"])))
                else:
                    print("n %d S %d mode %d: rows %d / %d" % (n, S, mode, a["best_row"], b["best_row"]))
                if mode == R.LMEDS and len(a["trace_score"]):
                    trace = max(trace, float(np.abs(a["trace_score"] - b["trace_score"]).max()))
                elif len(a["trace_score"]):
                    nd = int((a["trace_score"] != b["trace_score"]).sum())
                    if nd:
                        print("n %d S %d: %d inlier counts differ" % (n, S, nd))
    print("best model / score: %.3g   per-row penalties: %.3g" % (best, trace))


if __name__ == "__main__":
    measure_float64_error()
