"""CPU checks of tests/camera_cases.py on the oracle alone: the conditions the GPU tests of the camera axis rely on, so that an empty
case cannot pass silently.  The numpy restatement of the fisheye Newton loop equals the oracle; fisheye_fold populates both failure
kinds and the success path on the key-point sets the GPU tests use; fisheye_wide reaches the clamp, undistorts everything and
inverts the forward model; the share of points on which tan's last bit decides the float pixel is what DESIGN.md section 2 states."""
import numpy as np
import pytest

from ov2slam_amd import synth
from tests import camera_cases as CC
from tests.test_oracle_undistort import distort_fisheye

FISHEYES = [n for n in CC.NAMES if CC.model(n) == "fisheye"]
SIZES = (1, 308, 5000)                                            # tests/test_gpu_keypoint.py


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_table():
    assert CC.NAMES == ("pinhole0", "radtan4", "radtan5", "rational8", "prism12", "fisheye_mild", "fisheye_wide", "fisheye_fold")
    assert [0 if CC.coeffs(n) is None else len(CC.coeffs(n)) for n in CC.NAMES] == [0, 4, 5, 8, 12, 4, 4, 4]
    for n in CC.NAMES:
        P = CC.params(n)
        assert P["model"] == CC.model(n) and P["K"] == CC.intrinsics(n) and P["D"] == CC.coeffs(n) and (P["img_w"], P["img_h"]) == (376, 240)


def test_every_pinhole_coefficient_count_gives_another_result(oracle):
    px = CC.points(308, 308)
    got = [_bits(CC.oracle_keypoints(oracle, n, px)[0]) for n in CC.NAMES if CC.model(n) == "pinhole"]
    for i in range(len(got)):
        for j in range(i):
            assert (got[i] != got[j]).any(axis=1).mean() > 0.5


@pytest.mark.parametrize("name", FISHEYES)
def test_numpy_restatement_equals_the_oracle(oracle, name):
    """failed set, pixels and bearings as bits: camera_cases.fisheye_newton is the oracle's loop, and says which reason applied"""
    for n in SIZES:
        px = CC.points(n, n)
        nw = CC.fisheye_newton(name, px)
        ru, rb = CC.oracle_keypoints(oracle, name, px)
        assert np.array_equal((ru == CC.FAIL_PX).all(axis=1), nw["kind"] != CC.OK)
        mine = CC.fisheye_pixels(name, nw)
        assert np.array_equal(_bits(mine), _bits(ru))
        assert np.array_equal(CC.bearings(name, mine).view(np.uint64), rb.view(np.uint64))


def test_fold_populates_both_failure_kinds_and_the_success_path():
    for n in SIZES[1:]:
        assert CC.fold_populated(CC.points(n, n)), CC.population("fisheye_fold", CC.points(n, n))
    nw = CC.fisheye_newton("fisheye_fold", CC.points(5000, 5000))
    r = np.hypot(*(nw["pw"] * 190.0).T)
    assert r[nw["kind"] == CC.OK].max() < 103.5 and r[nw["kind"] != CC.OK].min() > 103.0     # the fold at theta_d = 0.5443
    assert nw["trips"][nw["kind"] == CC.NOT_CONVERGED].min() == 10


def test_fold_is_populated_on_the_tracked_sets_of_the_gpu_tests(oracle):
    """The fused and stateful tests undistort what the tracker hands out.  The oracle's tracker gives the same positions bit for bit
    (tests/test_gpu_tracker.py), so their populations can be counted here: one key point per 15 px cell, ~400 an item, as
    test_tracker_computes_keypoints_under_every_camera and test_lockstep_p3p_rule_under_added_cameras draw them -- all three outcomes
    per item, and failed and successful undistortions in the set the p3p rule runs again."""
    from tests.test_gpu_tracker import _oracle_frame, _points, _sequence
    w, h = CC.W, CC.H
    views, flow = _sequence(w, h, 3, seed=21)
    rng = np.random.default_rng(6)
    for cap in (512, 100):
        kps, pri, hp = _points(w, h, flow, 0, rng, 1.0, bad_frac=0.25, cell=15)
        assert len(kps) > 3 * 100
        assert CC.fold_populated(_oracle_frame(oracle, views[0], views[1], kps, pri, hp, False, w, h)[0])
        kps, pri, hp = _points(w, h, flow, 1, rng, 1.0, frac_prior=0.8, bad_frac=0.95, bad_sigma=60.0, cell=15)
        out, ok, rerun, p3p = _oracle_frame(oracle, views[1], views[2], kps, pri, hp, False, w, h)
        kind = CC.fisheye_kinds("fisheye_fold", out[rerun])
        assert p3p and CC.fold_populated(out) and (kind == CC.OK).sum() >= 20 and (kind != CC.OK).sum() >= 20
    seqs = [_sequence(w, h, 2, seed=70 + b) for b in range(3)]
    rng = np.random.default_rng(9)
    for b in range(3):
        kps, pri, hp = _points(w, h, seqs[b][1], 0, rng, 1.0, frac_prior=0.8, bad_frac=0.85 if b == 1 else 0.1, bad_sigma=40.0, cell=15)
        out, ok, rerun, p3p = _oracle_frame(oracle, seqs[b][0][0], seqs[b][0][1], kps, pri, hp, False, w, h)
        assert p3p == (b == 1) and CC.fold_populated(out)
        if b == 1:
            kind = CC.fisheye_kinds("fisheye_fold", out[rerun])
            assert (kind == CC.OK).sum() >= 20 and (kind != CC.OK).sum() >= 20
    # the 15 px grid itself, wherever a track moves it by a few pixels (test_lockstep_equals_single_trackers_under_added_cameras)
    for seed in range(100, 105):
        k = synth.grid_keypoints(w, h, 15, np.random.default_rng(seed))
        for shift in (0.0, 5.0, -5.0):
            assert CC.fold_populated(k[:len(k) - 28] + np.float32(shift))


def test_wide_reaches_the_clamp_and_undistorts_everything(oracle):
    for n in SIZES[1:]:
        px = CC.points(n, n)
        nw = CC.fisheye_newton("fisheye_wide", px)
        assert nw["clamped"].any() and (nw["kind"] == CC.OK).all()
        ru, _ = CC.oracle_keypoints(oracle, "fisheye_wide", px)
        assert not (ru == CC.FAIL_PX).any() and np.isfinite(ru).all()
    assert CC.fisheye_newton("fisheye_mild", CC.points(5000, 5000))["trips"].max() <= nw["trips"].max()


@pytest.mark.parametrize("name", ["fisheye_mild", "fisheye_wide"])
def test_oracle_inverts_the_forward_model(oracle, name):
    """As tests/test_oracle_undistort.py: distort, round to a float pixel, undistort.  The float pixel's half ulp (1.5e-5 px) comes
    back multiplied by d tan / d theta = 1 + r^2, so the file's 2e-3 px holds for r^2 < 60; the points are drawn with
    theta < 1.4 rad (r^2 < 34), which still covers distorted pixels over the whole frame for f = 140."""
    fx, fy, cx, cy = CC.intrinsics(name)
    rng = np.random.default_rng(1)
    th, phi = rng.uniform(0, 1.4, 4000), rng.uniform(0, 2 * np.pi, 4000)
    xn, yn = np.tan(th) * np.cos(phi), np.tan(th) * np.sin(phi)
    xd, yd = distort_fisheye(xn, yn, CC.coeffs(name))
    px = np.stack([xd * fx + cx, yd * fy + cy], 1)
    inside = (px[:, 0] > -10) & (px[:, 0] < CC.W + 10) & (px[:, 1] > -10) & (px[:, 1] < CC.H + 10)
    px, und = px[inside].astype(np.float32), np.stack([xn * fx + cx, yn * fy + cy], 1)[inside]
    assert len(px) > 400
    if name == "fisheye_wide":
        assert np.hypot(px[:, 0] - cx, px[:, 1] - cy).max() > 180        # out to the corners of the frame
    unpx, _ = CC.oracle_keypoints(oracle, name, px)
    assert np.abs(unpx - und).max() < 2e-3


@pytest.mark.parametrize("name", FISHEYES)
def test_tan_sensitive_share(name):
    """The share of points whose float pixel moves with tan's last bit: the cap of tests/test_gpu_keypoint.py, far below the flat
    1 % it replaces (DESIGN.md section 2 quotes these figures)."""
    px = CC.points(5000, 5000)
    sens, ref = CC.tan_sensitive(name, px)
    ok = CC.fisheye_kinds(name, px) == CC.OK
    print("%s: %d of %d successful points are tan-sensitive" % (name, sens.sum(), ok.sum()))
    assert not (sens & ~ok).any()
    assert sens.sum() < 0.01 * ok.sum()
