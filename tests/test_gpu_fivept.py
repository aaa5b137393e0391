"""The device 5-point essential-matrix search (csrc/fivept.hip, ov2_epipolar_ransac[_batch]) against the numpy specification
(tests/fivept_ref.py; OpenGV's solver and loop restated, not an OpenGV binary).

DECISIONS are compared exactly: status, iterations, rows consumed, best row, the outlier list, and every row's valid flag and
inlier count.  NUMBERS (every row's model and the final model) must lie within

    max(1e-12, 100 x |float64 - longdouble| of the specification on that row)

so the bound follows each row's conditioning (the degree-10 polynomial sets it: the difference spans 1e-15 .. 2e-4 over the
committed cases, median 1e-14, p99 8e-9; one global figure would be set by the tail); 1e-12 is a few thousand roundings of
entries of order 1, for rows on which the two precisions happen to agree to the last bits.  The device evaluates the same
operations as the specification in another order, hence 100 x.

CONDITIONS.  A row is FRAGILE when float64 and longdouble decide differently on it (validity, number of real roots, chosen (root,
candidate), inlier count) or when a point's distance lies within 1e-6 threshold of the threshold: such a row is compared on
nothing.  The seeds below are chosen so that no fragile row lies among the rows the specification's loop consumes, and at most 1 %
of all rows of the module are fragile; both are asserted."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import fivept_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TH = R.threshold_of(3.0, 460.0, 460.0)
NS = (8, 9, 63, 64, 65, 130, 513)               # 63 / 64 / 65: one wavefront of points and its neighbours; 513: nine strides
SS = (1, 65, 200)                               # 1, and two / seven work-groups of the solver with a partial last one
OUTLIERS = {8: 0.0, 9: 0.0, 63: 0.1, 64: 0.2, 65: 0.3, 130: 0.4, 513: 0.25}
FLOOR = 1e-12

_cache = {}


def scene(n, S):
    """the committed case (n, S): 0.5 px noise, 0 - 40 % outliers, the table of seed 1000 n + S, the specification's evaluation of
    every row in float64 and in longdouble, the fragile flags, the search"""
    key = (n, S)
    if key not in _cache:
        rng = np.random.default_rng(200000 + 1000 * n + S)
        bv1, bv2, Rw, t, planted = R.make_scene(rng, n, noise_px=0.5, outlier_frac=OUTLIERS[n])
        sm = R.draw_samples(1000 * n + S, n, S)
        c = dict(bv1=bv1, bv2=bv2, samples=sm, Rw=Rw, t=t, planted=planted)
        _finish_case(c, S)
        _cache[key] = c
    return _cache[key]


def _finish_case(c, max_iterations):
    c["prep"] = R.prepare(c["bv1"], c["bv2"], c["samples"])
    c["prep_ld"] = R.prepare(c["bv1"], c["bv2"], c["samples"], np.longdouble)
    c["fragile"] = R.fragile_rows(c["prep"], c["prep_ld"], TH)
    c["want"] = R.search(c["bv1"], c["bv2"], c["samples"], max_iterations, TH, prep=c["prep"])
    S = len(c["samples"])
    c["row_tol"] = np.full(S, FLOOR)
    for r in range(S):
        a, b = c["prep"][0][r], c["prep_ld"][0][r]
        if a is not None and b is not None:
            c["row_tol"][r] = max(FLOOR, 100.0 * float(np.abs(a - b).max()))
    return c


_worst = {"ratio": 0.0, "abs": 0.0}


def _compare(c, got):
    want, frag = c["want"], c["fragile"]
    consumed = np.asarray(want["consumed_rows"], np.int64)
    assert not frag[consumed].any(), "a fragile row among the rows the loop consumes: choose another seed"
    keep = ~frag
    assert np.array_equal(got["trace_valid"][keep], want["trace_valid"][keep])
    assert np.array_equal(got["trace_score"][keep], want["trace_score"][keep])
    for r in np.nonzero(keep & (want["trace_valid"] > 0))[0]:
        d = float(np.abs(got["trace_model"][r] - want["trace_model"][r]).max())
        _worst["abs"] = max(_worst["abs"], d)
        _worst["ratio"] = max(_worst["ratio"], d / c["row_tol"][r])
        assert d <= c["row_tol"][r], "row %d: model differs by %.3g, allowed %.3g" % (r, d, c["row_tol"][r])
    assert not got["trace_model"][keep & (want["trace_valid"] == 0)].any()
    assert got["status"] == want["status"]
    assert got["iterations"] == want["iterations"] and got["rows_consumed"] == want["rows_consumed"]
    assert got["best_row"] == want["best_row"]
    assert got["outliers"].dtype == np.int32 and np.array_equal(got["outliers"], want["outliers"])
    assert got["n_inliers"] == want["n_inliers"] == (len(c["bv1"]) - len(want["outliers"]) if want["best_row"] >= 0 else 0)
    if want["best_row"] >= 0:
        assert got["score"] == float(want["score"])
        assert np.abs(got["model"] - want["model"]).max() <= c["row_tol"][want["best_row"]]
        assert np.array_equal(got["model"], got["trace_model"][got["best_row"]])
    else:
        assert not got["model"].any() and len(got["outliers"]) == 0
    print("largest device - specification model difference so far %.3g (%.3g of its row's bound)" % (_worst["abs"], _worst["ratio"]))


@pytest.mark.gpu
@pytest.mark.parametrize("S", SS)
@pytest.mark.parametrize("n", NS)
def test_against_the_specification(gpu_ctx, n, S):
    from ov2slam_amd import pose
    c = scene(n, S)
    got = pose.epipolar_ransac(gpu_ctx, pose.epipolar_params(S, TH), c, trace=True)
    _compare(c, got)
    if S > 1 and n >= 63:
        assert got["ok"]
        assert set(np.nonzero(c["planted"])[0]) <= set(got["outliers"].tolist())                 # displaced across the epipolar line


@pytest.mark.gpu
def test_fragile_rows_are_rare():
    """after the cases above (shared cache): at most 1 % of all rows of the module are fragile"""
    nf = sum(int(scene(n, S)["fragile"].sum()) for n in NS for S in SS)
    nr = sum(S for n in NS for S in SS)
    print("fragile rows: %d of %d" % (nf, nr))
    assert nf <= 0.01 * nr


def _mixed_problems():
    out = []
    for n, S in ((130, 65), (0, 0), (7, 3), (65, 200), (9, 65), (513, 1), (7, 0), (64, 65), (8, 1), (0, 0), (63, 200)):
        if n >= 8:
            c = scene(n, S)
            out.append(dict(bv1=c["bv1"], bv2=c["bv2"], samples=c["samples"]))
        else:
            bv = np.tile([0, 0, 1.0], (n, 1))
            out.append(dict(bv1=bv, bv2=bv, samples=np.tile(np.arange(8, dtype=np.int32), (S, 1))))
    return out


def _same_bytes(a, b):
    for k in ("model", "trace_score", "trace_model"):
        assert np.array_equal(np.ascontiguousarray(a[k]).view(np.uint64), np.ascontiguousarray(b[k]).view(np.uint64)), k
    assert np.array_equal(np.float64(a["score"]).view(np.uint64), np.float64(b["score"]).view(np.uint64))
    for k in ("outliers", "trace_valid"):
        assert np.array_equal(a[k], b[k]), k
    for k in ("best_row", "iterations", "rows_consumed", "status", "n_inliers"):
        assert a[k] == b[k], k


@pytest.mark.gpu
def test_batch_equals_single_calls(gpu_ctx):
    """a mixed batch, among it empty and 7-point items: per item the batch form gives the single call's bytes"""
    from ov2slam_amd import pose
    P = pose.epipolar_params(100, TH)
    pbs = _mixed_problems()
    batch = pose.epipolar_ransac_batch(gpu_ctx, P, pbs, trace=True)
    assert len(batch) == len(pbs)
    for pb, b in zip(pbs, batch):
        _same_bytes(pose.epipolar_ransac(gpu_ctx, P, pb, trace=True), b)
        if len(pb["bv1"]) < 8:
            assert b["status"] == pose.EPI_TOO_FEW_POINTS and b["best_row"] == -1 and len(b["outliers"]) == 0 and b["iterations"] == 0
            assert b["rows_consumed"] == 0 and b["n_inliers"] == 0 and not b["model"].any()
        else:
            assert b["best_row"] >= 0
    assert pose.epipolar_ransac_batch(gpu_ctx, P, []) == []


@pytest.mark.gpu
def test_two_runs_give_identical_bytes(gpu_ctx):
    from ov2slam_amd import pose
    P = pose.epipolar_params(200, TH)
    pbs = _mixed_problems()
    a, b = pose.epipolar_ransac_batch(gpu_ctx, P, pbs, trace=True), pose.epipolar_ransac_batch(gpu_ctx, P, pbs, trace=True)
    for x, y in zip(a, b):
        _same_bytes(x, y)


def _crafted(c, sm, max_iterations=50):
    return _finish_case(dict(bv1=c["bv1"], bv2=c["bv2"], samples=np.asarray(sm, np.int32)), max_iterations)


@pytest.mark.gpu
def test_crafted_cases(gpu_ctx):
    from ov2slam_amd import pose
    P = pose.epipolar_params(50, TH)
    c = scene(65, 65)
    # every row invalid: a repeated index, an index out of range on either side
    bad = np.array([[1, 1, 2, 3, 4, 5, 6, 7], [0, 1, 2, 3, 4, 5, 6, 65], [-1, 2, 3, 4, 5, 6, 7, 8], [7, 8, 9, 10, 11, 12, 13, 7],
                    [0, 1, 2, 3, 4, 5, 6, 2 ** 31 - 1], [-2 ** 31, 1, 2, 3, 4, 5, 6, 7]], np.int32)
    cc = _crafted(c, bad)
    got = pose.epipolar_ransac(gpu_ctx, P, cc, trace=True)
    assert cc["want"]["status"] == R.NO_MODEL | R.FEW_INLIERS and not cc["fragile"].any()
    _compare(cc, got)
    assert got["rows_consumed"] == 6 and got["iterations"] == 0 and not got["trace_valid"].any() and got["best_row"] == -1
    # repeated and out-of-range rows first, then good rows: the skipped rows count no iteration
    cc = _crafted(c, np.concatenate([bad[:3], c["samples"][:20]]))
    got = pose.epipolar_ransac(gpu_ctx, P, cc, trace=True)
    assert list(cc["want"]["trace_valid"][:3]) == [0, 0, 0] and cc["want"]["trace_valid"][3:].all()
    _compare(cc, got)
    assert got["rows_consumed"] == got["iterations"] + 3
    # pure outliers: bearings that have nothing to do with each other
    rng = np.random.default_rng(11)
    n = 40
    bv1, bv2 = rng.normal(size=(n, 3)) + [0, 0, 3], rng.normal(size=(n, 3)) + [0, 0, 3]
    bv1 /= np.sqrt((bv1 * bv1).sum(axis=1))[:, None]
    bv2 /= np.sqrt((bv2 * bv2).sum(axis=1))[:, None]
    cc = _finish_case(dict(bv1=bv1, bv2=bv2, samples=R.draw_samples(4, n, 30)), 50)
    assert cc["want"]["status"] == R.FEW_INLIERS
    got = pose.epipolar_ransac(gpu_ctx, P, cc, trace=True)
    _compare(cc, got)
    assert not got["ok"]


@pytest.mark.gpu
def test_zero_parallax_and_too_few_points(gpu_ctx):
    """bv1 == bv2: the rays are parallel, every quantity of the solver is degenerate (the constraints hold for E = [t]x with any
    t); nothing is compared with the specification, the call returns and reports a defined state.  n < 8: TOO_FEW_POINTS alone."""
    from ov2slam_amd import pose
    P = pose.epipolar_params(50, TH)
    c = scene(65, 65)
    got = pose.epipolar_ransac(gpu_ctx, P, dict(bv1=c["bv1"], bv2=c["bv1"], samples=c["samples"]), trace=True)
    assert got["status"] in (0, pose.EPI_FEW_INLIERS, pose.EPI_NO_MODEL | pose.EPI_FEW_INLIERS)
    assert (got["best_row"] < 0) == bool(got["status"] & pose.EPI_NO_MODEL)
    assert (got["n_inliers"] < 10) == bool(got["status"] & pose.EPI_FEW_INLIERS)
    assert np.isfinite(got["model"]).all() and np.isfinite(got["trace_model"]).all()
    assert got["n_inliers"] + len(got["outliers"]) == (65 if got["best_row"] >= 0 else 0)
    assert 0 <= got["iterations"] <= got["rows_consumed"] <= 65
    for n in (0, 1, 7):
        got = pose.epipolar_ransac(gpu_ctx, P, dict(bv1=c["bv1"][:n], bv2=c["bv2"][:n], samples=c["samples"]), trace=True)
        want = R.search(c["bv1"][:n], c["bv2"][:n], c["samples"], 50, TH)
        assert got["status"] == want["status"] == R.TOO_FEW_POINTS and got["best_row"] == -1 and got["iterations"] == 0
        assert got["rows_consumed"] == 0 and len(got["outliers"]) == 0 and not got["trace_valid"].any() and not got["model"].any()


@pytest.mark.gpu
def test_invalid_arguments_with_a_context(gpu_ctx):
    from ov2slam_amd import pose, _lib as L
    c = scene(9, 1)
    for kw in (dict(threshold=0.0), dict(threshold=float("nan")), dict(boptimize=True), dict(max_iterations=-1), dict(probability=1.0)):
        args = dict(max_iterations=10, threshold=TH)
        args.update(kw)
        with pytest.raises(L.Ov2Error) as e:
            pose.epipolar_ransac(gpu_ctx, pose.epipolar_params(**args), c)
        assert e.value.code == L.OV2_EINVAL
    bv2 = c["bv2"].copy()
    bv2[3, 1] = np.inf
    with pytest.raises(L.Ov2Error):
        pose.epipolar_ransac(gpu_ctx, pose.epipolar_params(10, TH), dict(c, bv2=bv2))


@pytest.mark.gpu
def test_tracker_bearings_to_epipolar(gpu_ctx):
    """the chain VisualFrontEnd::epipolar2d2dFiltering runs: the tracker's bearing vectors of the keyframe's and of the current
    frame's keypoints (ov2_tracker_last_keypoints) go through epipolar_ransac.  Synthetic scene with a known relative pose and 25
    planted mismatches; the decisions are the specification's on the same bearings, the pose is the scene's within the bound the
    specification reaches."""
    import ov2slam_amd
    from ov2slam_amd import pose, synth
    w, h, K = 376, 240, (300.0, 300.0, 188.0, 120.0)
    rng = np.random.default_rng(33)
    n0 = 140
    Rw = R._rot(rng, 0.08)
    t = np.array([0.9, 0.1, 0.2])
    t /= np.sqrt((t * t).sum())
    px2 = np.stack([rng.uniform(40, w - 40, n0), rng.uniform(40, h - 40, n0)], axis=1)
    depth = rng.uniform(4.0, 9.0, n0)
    x2 = np.stack([(px2[:, 0] - K[2]) / K[0] * depth, (px2[:, 1] - K[3]) / K[1] * depth, depth], axis=1)
    x1 = x2 @ Rw.T + t
    px1 = np.stack([K[0] * x1[:, 0] / x1[:, 2] + K[2], K[1] * x1[:, 1] / x1[:, 2] + K[3]], axis=1)
    planted = np.zeros(n0, bool)
    planted[rng.choice(n0, 25, replace=False)] = True
    px1[planted, 1] += rng.choice([-1.0, 1.0], 25) * rng.uniform(15, 30, 25)     # t is nearly along x: across the epipolar lines
    inside = (px1[:, 0] > 20) & (px1[:, 0] < w - 20) & (px1[:, 1] > 20) & (px1[:, 1] < h - 20)
    px1, px2, planted = px1[inside], px2[inside], planted[inside]
    n = len(px1)
    assert n >= 100
    px1 = (px1 + rng.normal(0, 0.3, px1.shape)).astype(np.float32)
    px2 = (px2 + rng.normal(0, 0.3, px2.shape)).astype(np.float32)
    img = synth.frame_pair(w, h, seed=3)[0]
    bvs = []
    for px in (px1, px2):
        vt = ov2slam_amd.VisualFrontEndTracker(gpu_ctx, w, h, use_clahe=False, nbmaxkps=256)
        vt.setCalibration(ov2slam_amd.CameraCalibration(gpu_ctx, "pinhole", *K))
        vt.trackFrame(img, np.zeros((0, 2), np.float32), np.zeros((0, 2), np.float32), None)
        out, st, _ = vt.trackFrame(img, px, px, np.ones(n, np.uint8))       # the same image: a tracked point stays where it is
        _, bv = vt.lastKeypoints(n)
        vt.close()
        bvs.append((np.asarray(bv, np.float64), (st & 1) > 0, out))
    good = bvs[0][1] & bvs[1][1]
    assert good.sum() >= 80 and np.abs(bvs[0][2][good] - px1[good]).max() < 0.05
    bv1, bv2, planted = bvs[0][0][good], bvs[1][0][good], planted[good]
    th = pose.epipolar_threshold(3.0, K[0], K[1])
    assert th == R.threshold_of(3.0, K[0], K[1])
    cc = dict(bv1=bv1, bv2=bv2, samples=R.draw_samples(5, len(bv1), 100))
    cc["prep"] = R.prepare(bv1, bv2, cc["samples"])
    want = R.search(bv1, bv2, cc["samples"], 100, th, prep=cc["prep"])
    frag = R.fragile_rows(cc["prep"], R.prepare(bv1, bv2, cc["samples"], np.longdouble), th)
    assert not frag[np.asarray(want["consumed_rows"], np.int64)].any(), "a fragile row among the rows the loop consumes"
    got = pose.epipolar_ransac(gpu_ctx, pose.epipolar_params(100, th), cc, trace=True)
    assert got["ok"] and got["best_row"] == want["best_row"] and np.array_equal(got["outliers"], want["outliers"])
    assert got["iterations"] == want["iterations"]
    assert set(np.nonzero(planted)[0]) <= set(got["outliers"].tolist())
    bound = max(np.abs(want["model"][:9].reshape(3, 3) - Rw).max(), np.abs(want["model"][9:] - t).max())
    print("specification's pose error on this scene %.3g" % bound)
    assert bound < 0.1
    assert np.abs(got["Rwc"] - Rw).max() <= bound + 1e-6 and np.abs(got["twc"] - t).max() <= bound + 1e-6


def _wr(f, a):
    a = np.ascontiguousarray(a)
    f.write(struct.pack("<q", a.nbytes)); f.write(a.tobytes())


def _rd(f, dt):
    nb = struct.unpack("<q", f.read(8))[0]
    return np.frombuffer(f.read(nb), dt)


@pytest.mark.gpu
def test_cpp_adapter(gpu_ctx, tmp_path):
    """tests/cpp/fivept_run.cpp: ov2::compute5ptEssentialMatrix returns the Python form's Rwc, twc, outliers and bool, with
    bdorandom (the caller's seed) and without (the fixed seed)"""
    from ov2slam_amd import pose
    exe = tmp_path / "fivept_run"
    libdir = os.path.join(ROOT, "ov2slam_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "fivept_run.cpp"),
                           "-o", str(exe), "-L", libdir, "-lov2slam_hip", "-Wl,-rpath," + libdir])
    c = scene(130, 65)
    n, seed, nmaxiter, errth, fx, fy = 130, 77, 100, 3.0, 458.654, 457.296
    case, res = tmp_path / "case.bin", tmp_path / "res.bin"
    with open(case, "wb") as f:
        _wr(f, np.array([nmaxiter, seed], np.int32)); _wr(f, np.array([errth, fx, fy], np.float32)); _wr(f, c["bv1"]); _wr(f, c["bv2"])
    r = subprocess.run([str(exe), str(case), str(res)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    th = pose.epipolar_threshold(errth, fx, fy)
    with open(res, "rb") as f:
        for bdorandom in (1, 0):
            ok, Rwc, twc, out = _rd(f, np.int32), _rd(f, np.float64), _rd(f, np.float64), _rd(f, np.int32)
            sm = pose.epipolar_draw_samples(seed if bdorandom else 0, n, 2 * nmaxiter)
            py = pose.epipolar_ransac(gpu_ctx, pose.epipolar_params(nmaxiter, th), dict(bv1=c["bv1"], bv2=c["bv2"], samples=sm))
            assert bool(ok[0]) == py["ok"] and py["ok"]
            assert np.array_equal(out, py["outliers"])
            assert np.array_equal(Rwc.reshape(3, 3), py["Rwc"]) and np.array_equal(twc, py["twc"])
        small_ok, small_out = _rd(f, np.int32), _rd(f, np.int32)
        assert small_ok[0] == 0 and len(small_out) == 0                  # seven points: false, nothing written
