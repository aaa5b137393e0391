"""The camera table of the fused and stateful front-end tests (plain numpy): every model KpCalib carries -- the pinhole model with
0 / 4 / 5 / 8 / 12 coefficients and the 4-coefficient fisheye model -- for the 376 x 240 frame of tests/test_gpu_priors_lockstep.py.
What tests/test_camera_cases.py checks on the oracle alone and the test_gpu_* files run through the HIP kernels.

  pinhole0, radtan4            what ran before the table existed
  radtan5, rational8, prism12  k[4..11] reach the device through every host driver
  fisheye_mild                 the camera of the stand-alone priors / match / loop-map tests
  fisheye_wide                 f = 140 px: theta_d reaches the +-pi/2 clamp in the corners, where theta passes pi/2 and tan turns negative
  fisheye_fold                 theta (1 - 0.5 theta^2) has its maximum 0.5443 at theta = 0.8165: no solution beyond 103 px from the
                               centre.  There cv::fisheye::undistortPoints does not converge in 10 trips, or converges on a negative
                               theta ("flipped"), and undistortImagePoint hands out (-1e6, -1e6): the failure branch.

fisheye_kinds() restates the Newton loop of oracle/undistort.c in numpy, operation by operation, and says which of the two reasons
applied; tests/test_camera_cases.py holds it equal to the oracle."""
import math

import numpy as np

from tests.match_ref import FISHEYE4

W, H = 376, 240
K = (229.327, 228.648, 183.6075, 124.1875)                        # EuRoC halved
D4 = (-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05)
D5 = D4 + (0.01,)
D8 = D4 + (0.01, 0.02, -0.01, 0.005)
D12 = D8 + (1e-3, -2e-3, 1e-3, 5e-4)

# name -> (model, K, D)
CAMERAS = {
    "pinhole0":     ("pinhole", K, None),
    "radtan4":      ("pinhole", K, D4),
    "radtan5":      ("pinhole", K, D5),
    "rational8":    ("pinhole", K, D8),
    "prism12":      ("pinhole", K, D12),
    "fisheye_mild": ("fisheye", K, FISHEYE4),
    "fisheye_wide": ("fisheye", (140.0, 140.0, 188.0, 120.0), (0.0034, 0.0007, -0.0020, 0.0002)),
    "fisheye_fold": ("fisheye", (190.0, 190.0, 188.0, 120.0), (-0.5, 0.0, 0.0, 0.0)),
}
NAMES = tuple(CAMERAS)
ADDED = ("rational8", "fisheye_wide")                             # what every fused path runs beside its own camera
ADDED_FOLD = ADDED + ("fisheye_fold",)
FAIL_PX = np.float32(-1000000.0)
OK, NOT_CONVERGED, FLIPPED = 0, 1, 2
FOLD_MIN = {NOT_CONVERGED: 10, FLIPPED: 3, OK: 20}                # the least population of every kind, per item


def model(name):
    return CAMERAS[name][0]


def intrinsics(name):
    return CAMERAS[name][1]


def coeffs(name):
    return CAMERAS[name][2]


def calibration(ctx, name):
    """the ov2slam_amd.CameraCalibration of camera `name`"""
    import ov2slam_amd
    m, k, d = CAMERAS[name]
    return ov2slam_amd.CameraCalibration(ctx, m, *k, D=d)


def params(name):
    """the dict the priors, match and stereo parameter blocks take"""
    m, k, d = CAMERAS[name]
    return dict(model=m, K=k, D=d, img_w=W, img_h=H)


def iK(name):
    fx, fy, cx, cy = CAMERAS[name][1]
    return np.linalg.inv(np.array([[fx, 0., cx], [0., fy, cy], [0., 0., 1.]]))


def oracle_keypoints(O, name, px):
    """oracle.compute_keypoints under camera `name` -> (unpx, bv)"""
    m, k, d = CAMERAS[name]
    return O.compute_keypoints(O.CAM_FISHEYE if m == "fisheye" else O.CAM_PINHOLE, k, d, iK(name), px)


def points(n, seed):
    """n pixels over the frame and 10 px beyond every border (the stand-alone calls' inputs)"""
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(-10, W + 10, n), rng.uniform(-10, H + 10, n)], 1).astype(np.float32)


def fisheye_newton(name, px):
    """The loop of cv::fisheye::undistortPoints as oracle/undistort.c states it, in numpy doubles (no contraction), for float32 pixels.
    -> dict: kind (OK / NOT_CONVERGED / FLIPPED; a point that is both counts as NOT_CONVERGED), clamped, trips, theta, theta_d,
    pw (n,2)"""
    m, (fx, fy, cx, cy), k = CAMERAS[name]
    assert m == "fisheye"
    px = np.asarray(px, np.float32).reshape(-1, 2).astype(np.float64)
    EPS, PI_2 = 1e-8, 3.1415926535897932384626433832795 / 2.
    pwx, pwy = (px[:, 0] - cx) / fx, (px[:, 1] - cy) / fy
    raw = np.sqrt(pwx * pwx + pwy * pwy)
    theta_d = np.minimum(np.maximum(-PI_2, raw), PI_2)
    theta = theta_d.copy()
    small = ~(np.abs(theta_d) > EPS)
    converged = small.copy()
    trips = np.zeros(len(px), int)
    for _ in range(10):
        run = ~converged
        t = theta[run]
        t2 = t * t; t4 = t2 * t2; t6 = t4 * t2; t8 = t6 * t2
        a, b, c, d = k[0] * t2, k[1] * t4, k[2] * t6, k[3] * t8
        fix = (t * (1 + a + b + c + d) - theta_d[run]) / (1 + 3 * a + 5 * b + 7 * c + 9 * d)
        theta[run] = t - fix
        trips[run] += 1
        done = np.zeros(len(px), bool)
        done[run] = np.abs(fix) < EPS
        converged |= done
    flipped = ((theta_d < 0) & (theta > 0)) | ((theta_d > 0) & (theta < 0))
    kind = np.where(~converged, NOT_CONVERGED, np.where(flipped, FLIPPED, OK))
    return dict(kind=kind, clamped=raw > PI_2, trips=trips, theta=theta, theta_d=theta_d, pw=np.stack([pwx, pwy], 1), small=small)


def fisheye_kinds(name, px):
    return fisheye_newton(name, px)["kind"]


def fisheye_pixels(name, nw, nudge=0):
    """The undistorted float32 pixel of every OK point of fisheye_newton's result, tan(theta) moved by `nudge` double ulps
    (libm's tan through math.tan, as the oracle); failed points get (-1e6, -1e6)."""
    _, (fx, fy, cx, cy), _ = CAMERAS[name]
    ok = nw["kind"] == OK
    t = np.array([math.tan(v) for v in nw["theta"]])
    for _ in range(abs(nudge)):
        t = np.nextafter(t, np.inf if nudge > 0 else -np.inf)
    with np.errstate(divide="ignore", invalid="ignore"):
        scale = np.where(nw["small"], 0.0, t / nw["theta_d"])
    pux, puy = nw["pw"][:, 0] * scale, nw["pw"][:, 1] * scale
    prx = (0. + fx * pux) + 0. * puy + cx * 1.0
    pry = (0. + 0. * pux) + fy * puy + cy * 1.0
    prz = (0. + 0. * pux) + 0. * puy + 1. * 1.0
    out = np.stack([prx / prz, pry / prz], 1).astype(np.float32)
    out[~ok] = FAIL_PX
    return out


def tan_sensitive(name, px):
    """The points whose float pixel changes when tan(theta) moves by one double ulp either way: the only ones on which a device tan
    that is last-bit different from the host's may give another pixel.  -> (mask, reference pixels)"""
    nw = fisheye_newton(name, px)
    ref = fisheye_pixels(name, nw)
    m = np.zeros(len(ref), bool)
    for s in (-1, 1):
        m |= (fisheye_pixels(name, nw, s).view(np.uint32) != ref.view(np.uint32)).any(axis=1)
    return m, ref


def population(name, px):
    """{kind: count} of the fisheye outcomes of px"""
    kind = fisheye_kinds(name, px)
    return {k: int((kind == k).sum()) for k in (OK, NOT_CONVERGED, FLIPPED)}


def fold_populated(px):
    """every outcome of fisheye_fold is met often enough among px (FOLD_MIN)"""
    p = population("fisheye_fold", px)
    return all(p[k] >= FOLD_MIN[k] for k in FOLD_MIN)


def bearings(name, unpx):
    """iK (u, v, 1) normalised, in the oracle's operation order"""
    m = iK(name).reshape(9)
    u = np.asarray(unpx, np.float32).astype(np.float64)
    b = np.stack([(m[3 * r] * u[:, 0] + m[3 * r + 1] * u[:, 1]) + m[3 * r + 2] * 1. for r in range(3)], 1)
    nrm = np.sqrt((b[:, 0] * b[:, 0] + b[:, 1] * b[:, 1]) + b[:, 2] * b[:, 2])
    return b / nrm[:, None]


def assert_keypoints_match_oracle(O, name, px, unpx, bv):
    """The stand-alone bound of every camera: the pinhole models and every failed fisheye point as bits; a successful fisheye point
    may differ only where one double ulp on tan(theta) moves the float pixel, and then by one float ulp; bearings as bits wherever
    the pixel is equal.  -> number of differing points"""
    ru, rb = oracle_keypoints(O, name, px)
    unpx = np.ascontiguousarray(unpx, np.float32); bv = np.ascontiguousarray(bv)
    if model(name) != "fisheye":
        assert np.array_equal(unpx.view(np.uint32), ru.view(np.uint32)) and np.array_equal(bv.view(np.uint64), rb.view(np.uint64))
        return 0
    failed = (ru == FAIL_PX).all(axis=1)
    assert np.array_equal((unpx == FAIL_PX).all(axis=1), failed)
    sens, _ = tan_sensitive(name, px)
    differ = (unpx.view(np.uint32) != ru.view(np.uint32)).any(axis=1)
    assert not (differ & ~sens).any() and not (differ & failed).any()
    assert differ.sum() <= sens.sum()
    ulp = np.spacing(np.abs(ru))
    assert (np.abs(unpx.astype(np.float64) - ru) <= ulp)[differ].all()
    assert np.array_equal(bv[~differ].view(np.uint64), rb[~differ].view(np.uint64))
    return int(differ.sum())


def assert_step_anchor(ctx, O, cal, name, step, result):
    """What ties a fused lock-step step to the reference, after the step and for every item: lastKeypoints equals the stand-alone
    ov2_compute_keypoints on the item's output positions as bits (both are device code on the same input), that call equals the
    oracle within the camera's bound, and the priors derived on the device equal ov2_klt_priors_batch as bits.
    step: the arguments (kps, wpt, is3d, Tcw, n, klt_use_prior), result: out, kp = [lastKeypoints], pr = [lastPriors] per item."""
    from ov2slam_amd import priors as PR
    na = len(result["kp"])
    items = []
    for b in range(na):
        m = int(step["n"][b])
        out = np.ascontiguousarray(result["out"][b, :m])
        unpx, bv = result["kp"][b]
        if m:
            su, sb = cal.computeKeypoints(out)
            assert np.array_equal(unpx.view(np.uint32), su.view(np.uint32)) and np.array_equal(bv.view(np.uint64), sb.view(np.uint64)), b
            assert_keypoints_match_oracle(O, name, out, su, sb)
        if "Tcw" in step:
            items.append(dict(Tcw=step["Tcw"][b], px=step["kps"][b, :m], is3d=step["is3d"][b, :m], wpt=step["wpt"][b, :m]))
    if items and result.get("pr") is not None:
        host = PR.klt_priors_batch(ctx, dict(params(name), klt_use_prior=step.get("klt_use_prior", True)), items)
        for b in range(na):
            lp, lh = result["pr"][b]
            assert np.array_equal(lp.view(np.uint32), host[b]["prior"].view(np.uint32)) and np.array_equal(lh, host[b]["has_prior"]), b


FOLD_PEAK = math.sqrt(2. / 3.)                                    # theta at which theta (1 - 0.5 theta^2) peaks


def fold_ring_points(n, rng):
    """n key points for fisheye_fold, shuffled: half within 95 px of the centre (they undistort), half between 104 and 112 px from it
    (they fail), all at least 20 px inside the frame"""
    _, (fx, fy, cx, cy), _ = CAMERAS["fisheye_fold"]
    out = []
    for lo, hi, cnt in ((0., 95., n - n // 2), (104., 112., n // 2)):
        while cnt:
            r, phi = math.sqrt(rng.uniform(lo * lo, hi * hi)), rng.uniform(0, 2 * math.pi)
            x, y = cx + r * math.cos(phi), cy + r * math.sin(phi)
            if 20 <= x <= W - 20 and 20 <= y <= H - 20:
                out.append((x, y)); cnt -= 1
    return np.array(out, np.float32).reshape(-1, 2)[rng.permutation(n)]


def fold_rays(px, bv):
    """Camera rays (z = 1) whose projection under fisheye_fold lies on or next to px: bv / bv.z where px undistorts.  No ray projects
    beyond 103.4 px from the centre, so a failed point gets the ray at the fold's peak in its direction: its projection, the prior of
    the tracking step, lies within (radius - 103.4) px of px."""
    _, (fx, fy, cx, cy), _ = CAMERAS["fisheye_fold"]
    px = np.asarray(px, np.float32).reshape(-1, 2)
    rays = np.asarray(bv, np.float64) / np.asarray(bv, np.float64)[:, 2:3]
    failed = fisheye_kinds("fisheye_fold", px) != OK
    phi = np.arctan2((px[:, 1].astype(np.float64) - cy) / fy, (px[:, 0].astype(np.float64) - cx) / fx)
    peak = np.stack([math.tan(FOLD_PEAK) * np.cos(phi), math.tan(FOLD_PEAK) * np.sin(phi), np.ones(len(px))], 1)
    rays[failed] = peak[failed]
    return rays
