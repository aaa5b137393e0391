"""The numpy restatement of the mapper's triangulation (tests/tri_ref.py): triangulate2 against an independent least-squares
midpoint, exact recovery on noise-free scenes, the literal sequential replay of both reference loops (a) against the per-keypoint
form the kernel implements (b) -- the data-parallelism argument, checked -- and one crafted case per branch."""
import copy

import numpy as np
import pytest

from tests import tri_ref as R


def _lsq_midpoint(Rm, t, f1, f2):
    """argmin |l0 f1 - (t + l1 R f2)|^2 by numpy's least squares, then the midpoint of the two closest points"""
    f2u = np.asarray(Rm) @ np.asarray(f2)
    A = np.stack([np.asarray(f1), -f2u], 1)
    l, *_ = np.linalg.lstsq(A, np.asarray(t), rcond=None)
    return (l[0] * np.asarray(f1) + (np.asarray(t) + l[1] * f2u)) / 2


def test_triangulate2_equals_least_squares_midpoint():
    rng = np.random.default_rng(0)
    n = 0
    for _ in range(500):
        q = rng.normal(0, 0.2, 4); q[3] = 1.0; q /= np.linalg.norm(q)
        Rm = np.array(R.rotation_matrix(tuple(q)))
        t = rng.normal(0, 0.5, 3)
        X = rng.normal(0, 3, 3); X[2] = abs(X[2]) + 2
        f1 = X / np.linalg.norm(X) + rng.normal(0, 0.01, 3)                 # skew rays: the midpoint is not the point
        f1 /= np.linalg.norm(f1)
        f2 = Rm.T @ (X - t); f2 /= np.linalg.norm(f2)
        if np.linalg.norm(np.cross(f1, Rm @ f2)) < 0.05:                  # the normal equations lose digits as the rays turn parallel
            continue
        n += 1
        got = np.array(R.triangulate2(R.rotation_matrix(tuple(q)), tuple(t), tuple(f1), tuple(f2)))
        ref = _lsq_midpoint(Rm, t, f1, f2)
        assert np.linalg.norm(got - ref) <= 1e-12 * np.linalg.norm(ref), (got, ref)
    assert n > 300


def test_sophus_restatement_is_consistent():
    """se3_inv / se3_mul / rotation_matrix agree with their matrix meaning"""
    rng = np.random.default_rng(1)
    for _ in range(100):
        A = R._pose(rng.normal(0, 1, 3), R._quat(rng, 0.5))
        B = R._pose(rng.normal(0, 1, 3), R._quat(rng, 0.5))
        p = tuple(rng.normal(0, 2, 3))
        ab = R.se3_act(R.se3_mul(R.pose(A), R.pose(B)), p)
        assert np.allclose(ab, R.se3_act(R.pose(A), R.se3_act(R.pose(B), p)), atol=1e-12)
        assert np.allclose(R.se3_act(R.se3_inv(R.pose(A)), R.se3_act(R.pose(A), p)), p, atol=1e-12)
        assert np.allclose(R.matvec(R.rotation_matrix(R.pose(A)[1]), p), R.so3_act(R.pose(A)[1], p), atol=1e-12)


@pytest.mark.parametrize("stereo", [True, False])
def test_noise_free_scene_recovers_the_points(stereo):
    """unrectified stereo and temporal points of a noise-free scene land within 1e-9 (relative) of the truth"""
    P = R.make_params(R.EUROC, stereo=stereo, seed=2)
    M = R.make_map(P, np.random.default_rng(3), n=400, p_stereo=0.5, p_src=1.0, motion=0.5)
    kf, lmids, _ = R.inputs_from_map(M)
    st, w, inv = R.keyframe(P, kf)
    ok = (st & (R.ST_STEREO_OK | R.ST_TEMPORAL_OK)) > 0
    assert ok.mean() > 0.95 and (st & R.ST_STEREO_OK).any() == stereo and (st & R.ST_TEMPORAL_OK).any()
    for i in np.nonzero(ok)[0]:
        truth = M["mps"][lmids[i]]["wpt"]
        assert np.linalg.norm(w[i] - truth) <= 1e-9 * np.linalg.norm(truth), (i, w[i], truth)


CFG = [
    dict(cam=R.EUROC, stereo=True, rect=False),
    dict(cam=R.KITTI, stereo=True, rect=True),
    dict(cam=R.EUROC, stereo=False, rect=False),
]


@pytest.mark.parametrize("cfg", range(len(CFG)))
@pytest.mark.parametrize("seed", range(6))
def test_sequential_replay_equals_per_keypoint_form(cfg, seed):
    """(a) == (b): the actions, their order and the bits of every point, on randomised keyframes with outliers, points behind the
    camera, a no-motion source keyframe and keypoints the host rules out of the temporal pass"""
    c = CFG[cfg]
    P = R.make_params(c["cam"], stereo=c["stereo"], rect=c["rect"], seed=seed)
    rng = np.random.default_rng(100 + seed)
    M = R.make_map(P, rng, n=250, n_src=int(rng.integers(1, 7)), noise=0.4, behind=0.05, no_motion_kf=seed % 2 == 0,
                   kps_3d=0.05, lone=0.1, missing_src_kp=0.05, motion=float(rng.uniform(0.05, 0.6)))
    kf, lmids, _ = R.inputs_from_map(M)
    st, w, inv = R.keyframe(P, kf)
    b = R.actions_from_status(M["frame"]["kfid"], lmids, st, w, inv)
    a = R.replay(P, copy.deepcopy(M))
    assert a == b
    kinds = {x[0] for x in a}
    assert "update" in kinds and ("rm_obs" in kinds or "rm_stereo" in kinds)


@pytest.mark.parametrize("case", R.crafted_cases(), ids=lambda c: c[0])
def test_crafted_branch(case):
    name, P, kf, expected = case
    st, w, inv = R.keyframe(P, kf)
    assert int(st[0]) == expected, (name, int(st[0]))
    if name.endswith("_nan"):
        assert np.isnan(w[0]).all() and np.isnan(inv[0])
    elif expected & (R.ST_STEREO_OK | R.ST_TEMPORAL_OK):
        assert np.isfinite(w[0]).all() and inv[0] > 0


def test_stereo_rejection_then_temporal_success_in_the_replay():
    """the stereo pass leaves a rejected keypoint 2-D; the temporal pass then creates its point, anchored at the source"""
    name, P, kf, _ = [c for c in R.crafted_cases() if c[0] == "stereo_rejected_then_temporal_ok"][0]
    M = dict(frame=dict(kfid=5, Twc=kf["Twc"], Tcw=R._inv7(kf["Twc"]),
                        kps=[dict(lmid=7, unpx=kf["unpx"][0], bv=kf["bv"][0], is3d=False, is_stereo=True, runpx=kf["runpx"][0],
                                  rbv=kf["rbv"][0])]),
             kfs={2: dict(Twc=kf["src_Twc"][0], Tcw=kf["src_Tcw"][0], kps={7: dict(unpx=kf["src_unpx"][0], bv=kf["src_bv"][0])}),
                  5: dict(Twc=kf["Twc"], Tcw=R._inv7(kf["Twc"]), kps={})},
             mps={7: dict(is3d=False, obs={2, 5})})
    acts = R.replay(P, M)
    assert [x[0] for x in acts] == ["rm_stereo", "update"] and M["mps"][7]["is3d"]
