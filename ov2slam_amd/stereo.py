"""Host-side mirror of the data-parallel part of MapManager::stereoMatching
(/root/reference/src/map_manager.cpp:367-611) on top of the C ABI:

    priors   rectified pairs: FeatureTracker::getLineMinSAD on the coarsest level (:421-439)
    track    fbKltTracking(left pyramid, right pyramid) -- kps with a 3-D prior on 1 level first, the failures
             and everything else on the full pyramid (:497-565)
    gate     right keypoint undistorted, |dy| or Sampson distance <= 2 (:568-590)

The map look-ups around it (projecting map points, surrounding-keypoint depth priors, updateKeypointStereo)
stay on the host in the reference and are inputs / outputs here; the two kinds of prior have a device form of their own
(ov2slam_amd/priors.py: stereo_priors, whose prior / has_prior are the priors3d_xy / has_prior3d of stereo_match_arrays)."""
import numpy as np

from . import _lib as L
from .frontend import _ptr


def epipolar_check(ctx, rect, Frl, right_calib, lunpx, rkps):
    """map_manager.cpp:568-590.  right_calib: ov2slam_amd.CameraCalibration of the right camera.
    Returns (rkps_out, runpx, epi_err, ok)."""
    lunpx = np.ascontiguousarray(lunpx, dtype=np.float32).reshape(-1, 2)
    rk = np.array(rkps, dtype=np.float32).reshape(-1, 2).copy()
    n = len(rk)
    runpx = np.empty((n, 2), np.float32); err = np.empty(n, np.float32); ok = np.zeros(n, np.uint8)
    F = None if Frl is None else np.ascontiguousarray(Frl, dtype=np.float64).reshape(9)
    D = right_calib.D
    L.check(ctx.lib.ov2_stereo_epipolar_check(ctx.h, int(bool(rect)), _ptr(F) if F is not None else None, right_calib.model,
                                              _ptr(right_calib.K), _ptr(D) if D is not None else None, 0 if D is None else len(D),
                                              _ptr(lunpx), _ptr(rk), n, _ptr(runpx), _ptr(err), _ptr(ok)))
    return rk, runpx, err, ok.astype(bool)


def stereo_matching(tracker, leftpyr, rightpyr, kps_px, kps_unpx, right_calib, *, rect, Frl=None, nklt_win_size=9,
                    nklt_pyr_lvl=3, nklt_err=30.0, fmax_fbklt_dist=0.5, priors3d=None):
    """kps_px / kps_unpx: (n,2) left keypoints (distorted / undistorted).  priors3d: optional dict
    {index: (x, y)} of right-image priors for keypoints with a usable 3-D prior (:402-413, :468-480).
    Returns (stereo_ok (n,) bool, right_px (n,2) float32) -- what updateKeypointStereo receives (:584)."""
    ctx = tracker.ctx
    kps_px = np.ascontiguousarray(kps_px, dtype=np.float32).reshape(-1, 2)
    n = len(kps_px)
    priors3d = priors3d or {}
    idx3d = np.array(sorted(priors3d), dtype=np.int64)
    idx2d = np.array([i for i in range(n) if i not in priors3d], dtype=np.int64)
    pri2d = kps_px[idx2d].copy()
    if rect and len(idx2d):
        up = np.float32(2.0 ** nklt_pyr_lvl); down = np.float32(1.0) / up
        xp, _ = tracker.getLineMinSAD(leftpyr, rightpyr, nklt_pyr_lvl, kps_px[idx2d] * down, 7, True)
        xp = xp * up                                                       # :433
        use = (xp >= 0) & (xp <= kps_px[idx2d, 0])                         # :435
        pri2d[use, 0] = xp[use]
    good_idx, good_r = [], []
    if len(idx3d):                                                         # :497-541
        p3 = np.array([priors3d[i] for i in idx3d], np.float32)
        out, st = tracker.fbKltTracking(leftpyr, rightpyr, nklt_win_size, 1, nklt_err, fmax_fbklt_dist, kps_px[idx3d], p3)
        good_idx += list(idx3d[st]); good_r += list(out[st])
        # failures are retried from the first call's forward result: v3dpriors was updated in place (:533-538, feature_tracker.cpp:66)
        idx2d = np.concatenate([idx2d, idx3d[~st]]); pri2d = np.concatenate([pri2d, out[~st]])
    if len(idx2d):                                                         # :544-565
        out, st = tracker.fbKltTracking(leftpyr, rightpyr, nklt_win_size, nklt_pyr_lvl, nklt_err, fmax_fbklt_dist, kps_px[idx2d], pri2d)
        good_idx += list(idx2d[st]); good_r += list(out[st])
    ok = np.zeros(n, bool); right = np.zeros((n, 2), np.float32)
    if good_idx:
        gi = np.array(good_idx, np.int64); gr = np.array(good_r, np.float32).reshape(-1, 2)
        rk, _, _, eok = epipolar_check(ctx, rect, Frl, right_calib, np.asarray(kps_unpx, np.float32)[gi], gr)
        ok[gi] = eok; right[gi] = rk
    return ok, right


def stereo_match_arrays(tracker, leftpyr, rightpyr, kps_px, kps_unpx, priors3d_xy, has_prior3d, right_calib, *, rect, Frl=None,
                        nklt_win_size=9, nklt_pyr_lvl=3, nklt_err=30.0, fmax_fbklt_dist=0.5):
    """ov2_stereo_match on flat arrays: priors3d_xy (n,2) float32 (ignored where has_prior3d[i] == 0), has_prior3d (n,) uint8.
    Returns (stereo_ok (n,) bool, right_px (n,2) float32)."""
    ctx = tracker.ctx
    kps_px = np.ascontiguousarray(kps_px, dtype=np.float32).reshape(-1, 2)
    kps_unpx = np.ascontiguousarray(kps_unpx, dtype=np.float32).reshape(-1, 2)
    p3 = np.ascontiguousarray(priors3d_xy, dtype=np.float32).reshape(-1, 2)
    hp = np.ascontiguousarray(has_prior3d, dtype=np.uint8).reshape(-1)
    n = len(kps_px)
    if len(kps_unpx) != n or len(p3) != n or len(hp) != n:
        raise ValueError("stereo_match_arrays: arrays differ in length")
    right = np.zeros((n, 2), np.float32); ok = np.zeros(n, np.uint8)
    F = None if Frl is None else np.ascontiguousarray(Frl, dtype=np.float64).reshape(9)
    D = right_calib.D
    L.check(ctx.lib.ov2_stereo_match(ctx.h, leftpyr.h_pyr, rightpyr.h_pyr, int(nklt_win_size), int(nklt_pyr_lvl), int(tracker.nmax_iter),
                                     float(tracker.fmax_px_precision), float(nklt_err), float(fmax_fbklt_dist), int(bool(rect)),
                                     _ptr(F) if F is not None else None, right_calib.model, _ptr(right_calib.K),
                                     _ptr(D) if D is not None else None, 0 if D is None else len(D), _ptr(kps_px), _ptr(kps_unpx),
                                     _ptr(p3), _ptr(hp), n, _ptr(right), _ptr(ok)))
    return ok.astype(bool), right


def stereo_match_batch_arrays(tracker, leftpyr, rightpyr, n_items, n_max, kps_px, kps_unpx, priors3d_xy, has_prior3d, n, right_calib, *, rect,
                              Frl=None, nklt_win_size=9, nklt_pyr_lvl=3, nklt_err=30.0, fmax_fbklt_dist=0.5):
    """ov2_stereo_match_batch: items [0, n_items) of two batch pyramids in one call.  Arrays are (batch, n_max, ...) with n[b] valid rows.
    Returns (stereo_ok (batch, n_max) bool, right_px (batch, n_max, 2) float32); rows beyond n[b] are zero."""
    ctx = tracker.ctx
    kps_px = np.ascontiguousarray(kps_px, dtype=np.float32).reshape(-1, n_max, 2)
    kps_unpx = np.ascontiguousarray(kps_unpx, dtype=np.float32).reshape(-1, n_max, 2)
    p3 = np.ascontiguousarray(priors3d_xy, dtype=np.float32).reshape(-1, n_max, 2)
    hp = np.ascontiguousarray(has_prior3d, dtype=np.uint8).reshape(-1, n_max)
    nn = np.ascontiguousarray(n, np.int32)
    right = np.zeros(kps_px.shape, np.float32); ok = np.zeros(hp.shape, np.uint8)
    F = None if Frl is None else np.ascontiguousarray(Frl, dtype=np.float64).reshape(9)
    D = right_calib.D
    L.check(ctx.lib.ov2_stereo_match_batch(ctx.h, leftpyr.h_pyr, rightpyr.h_pyr, int(n_items), int(nklt_win_size), int(nklt_pyr_lvl), int(tracker.nmax_iter),
                                           float(tracker.fmax_px_precision), float(nklt_err), float(fmax_fbklt_dist), int(bool(rect)),
                                           _ptr(F) if F is not None else None, right_calib.model, _ptr(right_calib.K),
                                           _ptr(D) if D is not None else None, 0 if D is None else len(D), int(n_max), _ptr(kps_px), _ptr(kps_unpx),
                                           _ptr(p3), _ptr(hp), _ptr(nn), _ptr(right), _ptr(ok)))
    return ok.astype(bool), right


def stereo_matching_fused(tracker, leftpyr, rightpyr, kps_px, kps_unpx, right_calib, *, rect, Frl=None, nklt_win_size=9,
                          nklt_pyr_lvl=3, nklt_err=30.0, fmax_fbklt_dist=0.5, priors3d=None):
    """ov2_stereo_match: the same flow as stereo_matching() in ONE enqueue and ONE synchronisation (SAD priors, both
    fbKltTracking calls with the retry of failed 3-D-prior tracks, epipolar gate).  Same arguments, same return."""
    kps_px = np.ascontiguousarray(kps_px, dtype=np.float32).reshape(-1, 2)
    n = len(kps_px)
    hp = np.zeros(n, np.uint8); p3 = kps_px.copy()
    for i, xy in (priors3d or {}).items():
        hp[i] = 1; p3[i] = xy
    return stereo_match_arrays(tracker, leftpyr, rightpyr, kps_px, kps_unpx, p3, hp, right_calib, rect=rect, Frl=Frl,
                               nklt_win_size=nklt_win_size, nklt_pyr_lvl=nklt_pyr_lvl, nklt_err=nklt_err,
                               fmax_fbklt_dist=fmax_fbklt_dist)
