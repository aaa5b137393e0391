"""The lock-step step with the priors derived on the device (ov2_btracker_track_frame_map, csrc/trackb.hip + csrc/priors.hip)
against the same step fed from the host: tracker A takes the output of ov2_klt_priors_batch through ov2_btracker_track_frame,
tracker B takes the map points and the predicted poses.  Positions, status, p3p requests, the computeKeypoint outputs and the
priors that were used are byte-equal on every frame -- with items of 0, 37 and 64 keypoints among 64 slots, an item that ends
early, a frame whose predicted poses are wrong (the p3p retry runs in both trackers) and a frame without klt_use_prior."""
import numpy as np
import pytest

import ov2slam_amd
from ov2slam_amd import _lib as L
from ov2slam_amd import priors as PR
from tests import camera_cases as CC
from tests.match_ref import _inv_act, _rand_pose
from tests.test_gpu_tracker import _bits, _sequence

pytestmark = pytest.mark.gpu

W, H = 376, 240                                                   # the smallest frame of tests/test_gpu_lockstep.py
K = (229.327, 228.648, 183.6075, 124.1875)                        # EuRoC halved
DIST = (-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05)
BATCH, N_MAX, NFRAMES = 3, 64, 5                                  # frame 0 builds the pyramids, four frames are tracked
LENGTH = [5, 5, 3]                                                # the last item ends after two tracked frames
COUNTS = [64, 37, 0]


def _wrong(T, rng, fx=K[0]):
    """the pose turned by 0.15 rad about y (by more for a shorter focal length fx): projections land ~35 px away, mostly still inside
    the image"""
    half = 0.075 * (K[0] / fx)                                    # K[0] / K[0] == 1.0: the EuRoC case is what it was
    s, c = np.sin(half), np.cos(half)
    x, y, z, w = T[3:]
    q = np.array([c * x + s * z, c * y + s * w, c * z - s * x, c * w - s * y])      # (0, s, 0, c) * q
    return np.concatenate([T[:3] + rng.normal(0, 0.05, 3), q / np.linalg.norm(q)])


def test_map_form_equals_host_priors(gpu_ctx):
    _map_form(gpu_ctx, None, None)


@pytest.mark.parametrize("camera", CC.ADDED)
def test_map_form_equals_host_priors_under_added_cameras(gpu_ctx, oracle, camera):
    """The same sequence under the added cameras of tests/camera_cases.py: the fused prior kernel runs kp_project_dist's rational and
    fisheye branches, and both trackers' lastKeypoints equal the stand-alone call as bits and the oracle within the camera's bound."""
    _map_form(gpu_ctx, oracle, camera)


def _map_form(gpu_ctx, oracle, camera):
    seqs = [_sequence(W, H, NFRAMES, seed=70 + b) for b in range(BATCH)]
    rng = np.random.default_rng(11)
    cal = CC.calibration(gpu_ctx, camera) if camera else ov2slam_amd.CameraCalibration(gpu_ctx, "pinhole", *K, D=DIST)
    A = ov2slam_amd.LockstepTracker(gpu_ctx, BATCH, W, H, use_clahe=False, nbmaxkps=N_MAX)
    B = ov2slam_amd.LockstepTracker(gpu_ctx, BATCH, W, H, use_clahe=False, nbmaxkps=N_MAX)
    A.setCalibration(cal); B.setCalibration(cal)
    P = CC.params(camera) if camera else dict(model="pinhole", K=K, D=DIST, img_w=W, img_h=H)
    z2 = np.zeros((BATCH, N_MAX, 2), np.float32)
    first = [seqs[b][0][0] for b in range(BATCH)]
    A.trackFrame(first, z2, z2, None, np.zeros(BATCH, np.int32))
    out, st, p3p = B.trackFrameMap(first, z2, np.zeros((BATCH, N_MAX, 3)), np.zeros((BATCH, N_MAX), np.uint8),
                                   np.tile(np.array([0, 0, 0, 0, 0, 0, 1.0]), (BATCH, 1)), np.zeros(BATCH, np.int32))
    assert not st.any() and not p3p.any()                         # first frame: pyramids only
    seen_p3p = False
    for f in range(NFRAMES - 1):
        na = sum(1 for b in range(BATCH) if LENGTH[b] > f + 1)
        use_prior = f != 3
        kps = np.zeros((BATCH, N_MAX, 2), np.float32); wpt = np.zeros((BATCH, N_MAX, 3)); is3d = np.zeros((BATCH, N_MAX), np.uint8)
        Tcw = np.zeros((BATCH, 7)); n = np.zeros(na, np.int32)
        items = []
        for b in range(na):
            m = COUNTS[(b + f) % 3]
            n[b] = m
            k = np.stack([rng.uniform(20, W - 20, m), rng.uniform(20, H - 20, m)], 1).astype(np.float32)
            gt = (seqs[b][1](k.astype(np.float64), f, f + 1) + rng.normal(0, 0.7, (m, 2))).astype(np.float32)
            T = _rand_pose(rng)
            unpx, bv = cal.computeKeypoints(gt) if m else (None, np.zeros((0, 3)))
            d3 = (rng.uniform(size=m) < 0.75).astype(np.uint8)
            for i in range(m):                                    # the map point whose projection under T is the true position
                wpt[b, i] = _inv_act(T, bv[i] / bv[i][2] * rng.uniform(2, 10))
            if m:
                wpt[b, 0] = _inv_act(T, (30.0, 0.0, 1.0))         # one that projects outside: no prior
                d3[0] = 1
            kps[b, :m], is3d[b, :m] = k, d3
            Tcw[b] = _wrong(T, rng, cal.K[0]) if f == 1 else T    # frame 1: the motion model is wrong
            items.append(dict(Tcw=Tcw[b], px=k, is3d=d3, wpt=wpt[b, :m]))
        imgs = [seqs[b][0][f + 1] for b in range(na)]
        host = PR.klt_priors_batch(gpu_ctx, dict(P, klt_use_prior=use_prior), items)
        pri = np.zeros((BATCH, N_MAX, 2), np.float32); hp = np.zeros((BATCH, N_MAX), np.uint8)
        for b in range(na):
            pri[b, :n[b]], hp[b, :n[b]] = host[b]["prior"], host[b]["has_prior"]
            if n[b] and use_prior:
                assert 0 < host[b]["n_prior"] < n[b] and host[b]["has_prior"][0] == 0
        oa, sa, pa = A.trackFrame(imgs, kps, pri, hp, n, klt_use_prior=use_prior)
        ob, sb, pb = B.trackFrameMap(imgs, kps, wpt, is3d, Tcw, n, klt_use_prior=use_prior)
        assert np.array_equal(_bits(oa), _bits(ob)), "frame %d positions" % f
        assert np.array_equal(sa, sb), "frame %d status" % f
        assert np.array_equal(pa, pb), "frame %d p3p request" % f
        for b in range(na):
            m = int(n[b])
            ua, ba = A.lastKeypoints(b, m)
            ub, bb = B.lastKeypoints(b, m)
            assert np.array_equal(_bits(ua), _bits(ub)) and np.array_equal(ba.view(np.uint64), bb.view(np.uint64)), (f, b)
            if camera and m:
                su, sb = cal.computeKeypoints(ob[b, :m])
                assert np.array_equal(_bits(ub), _bits(su)) and np.array_equal(bb.view(np.uint64), sb.view(np.uint64)), (f, b)
                CC.assert_keypoints_match_oracle(oracle, camera, ob[b, :m], su, sb)
            lp, lh = B.lastPriors(b, m)
            assert np.array_equal(_bits(lp), _bits(host[b]["prior"])) and np.array_equal(lh, host[b]["has_prior"]), (f, b)
            la, lha = A.lastPriors(b, m)
            assert np.array_equal(_bits(la), _bits(lp)) and np.array_equal(lha, lh if use_prior else np.zeros(m, np.uint8)), (f, b)
            if m and f != 1:
                assert (sa[b, :m] & 1).mean() > 0.5, (f, b)       # the scene tracks
        if f == 1:
            # fewer than a third of the prior tracks survive: the retry without priors ran, in both trackers
            assert pa[[b for b in range(na) if n[b]]].all() and (sa[:na] & 2).any()
            seen_p3p = True
        else:
            assert not pa.any(), f
        if not use_prior:
            assert all(not B.lastPriors(b, int(n[b]))[1].any() for b in range(na))
    assert seen_p3p
    A.close(); B.close()


def test_map_form_needs_a_calibration_and_leaves_the_tracker_usable(gpu_ctx):
    views, flow = _sequence(W, H, 3, seed=5)
    t = ov2slam_amd.LockstepTracker(gpu_ctx, 1, W, H, use_clahe=False, nbmaxkps=N_MAX)
    z2, z3, z1 = np.zeros((1, N_MAX, 2), np.float32), np.zeros((1, N_MAX, 3)), np.zeros((1, N_MAX), np.uint8)
    I = np.array([[0, 0, 0, 0, 0, 0, 1.0]])
    with pytest.raises(ov2slam_amd.Ov2Error) as e:
        t.trackFrameMap([views[0]], z2, z3, z1, I, [0])
    assert e.value.code == L.OV2_EINVAL and "calibration" in str(e.value)
    t.trackFrame([views[0]], z2, z2, None, [0])                   # nothing was enqueued or counted: this is the first frame
    k = np.zeros((1, N_MAX, 2), np.float32)
    k[0, :10] = np.stack([np.linspace(40, 300, 10), np.linspace(40, 200, 10)], 1)
    gt = flow(k[0, :10].astype(np.float64), 0, 1).astype(np.float32)
    p = k.copy(); p[0, :10] = gt
    with pytest.raises(ov2slam_amd.Ov2Error):
        t.trackFrameMap([views[1]], k, z3, z1, I, [10])
    out, st, p3p = t.trackFrame([views[1]], k, p, np.ones((1, N_MAX), np.uint8), [10])
    assert (st[0, :10] & 1).sum() >= 8 and np.abs(out[0, :10] - gt)[(st[0, :10] & 1) > 0].max() < 1.0
    t.close()
