"""Host-side mirror of the mapper's keyframe triangulation (the reference's src/mapper.cpp:191-461) on top of the C ABI
(ov2_triangulate_keyframe[_batch], csrc/triangulate.hip):

    stereo     Mapper::triangulateStereo (:346-461): rectified depth from the disparity, or OpenGV's triangulate2 on (bv, rbv)
               through the extrinsic; depth and reprojection gates
    temporal   Mapper::triangulateTemporal (:191-344): triangulate2 against the first observer of the map point, the same gates,
               removeMapPointObs when a rejected point has > 20 px of rotation-compensated parallax

The map look-ups that pick the temporal candidates and their source keyframe (:243-295) and the map mutations themselves stay
on the host in the reference and are inputs / outputs here: `status` holds the OV2_TRI_* bits a caller replays.

A keyframe is a dict of numpy arrays named like the fields of ov2_tri_keyframe: Twc (7,), unpx (n,2), bv (n,3), and optionally
is_stereo (n,), runpx (n,2), rbv (n,3), src (n,) int (-1: no candidate), src_unpx (n,2), src_bv (n,3), src_Twc (m,7), src_Tcw (m,7).
Poses are [tx ty tz qx qy qz qw], as held by the Frame.

Local-map matching (Mapper::matchToMap, src/mapper.cpp:576-774; ov2_match_to_map[_batch], csrc/mapmatch.hip): match_params(),
match_to_map(), match_to_map_batch().  A keyframe is a dict of numpy arrays named like the fields of ov2_match_keyframe (the
counts follow from the array lengths): Tcw (7,), nb3dkps, kp_px (n_kp,2), kp_mp (n_kp,), cell_start (ncells+1,), cell_kp,
obs_start (n_mp+1,), obs_kfid, obs_kf, obs_px (n_obs,2), desc_start (n_mp+1,), desc (n_desc,32) uint8, kf_Tcw (n_kf,7),
lm_mp (n_lm,), lm_wpt (n_lm,3)."""
import ctypes as C

import numpy as np

from . import _lib as L
from . import _mapmatch

STEREO_TRIED, STEREO_OK = L.OV2_TRI_STEREO_TRIED, L.OV2_TRI_STEREO_OK
TEMPORAL_TRIED, TEMPORAL_OK = L.OV2_TRI_TEMPORAL_TRIED, L.OV2_TRI_TEMPORAL_OK
NO_MOTION, REMOVE_OBS = L.OV2_TRI_NO_MOTION, L.OV2_TRI_REMOVE_OBS


def tri_params(K, iK, Kr, Tlr, Tcic0, *, stereo, rect, fmax_reproj_err):
    """ov2_tri_params: left K (fx fy cx cy) and iK_ (3x3), right K, getExtrinsic() and Tcic0_ of the right camera, the
    SlamParams' stereo_, bdo_stereo_rect_ and fmax_reproj_err_"""
    p = L.TriParams()
    p.stereo, p.rect, p.fmax_reproj_err = int(bool(stereo)), int(bool(rect)), float(fmax_reproj_err)
    p.K[:] = [float(v) for v in np.asarray(K, np.float64).reshape(4)]
    p.iK[:] = [float(v) for v in np.asarray(iK, np.float64).reshape(9)]
    p.Kr[:] = [float(v) for v in np.asarray(Kr, np.float64).reshape(4)]
    p.Tlr[:] = [float(v) for v in np.asarray(Tlr, np.float64).reshape(7)]
    p.Tcic0[:] = [float(v) for v in np.asarray(Tcic0, np.float64).reshape(7)]
    return p


def stereo_keyframe_params(right_calib, tri, *, img_w, img_h, Tcic0, rect, Frl=None, ncellsize=35, nklt_win_size=9, nklt_pyr_lvl=3,
                           nmax_iter=30, fmax_px_precision=0.01, nklt_err=30.0, fmax_fbklt_dist=0.5):
    """ov2_stereo_keyframe_params of LockstepTracker.stereoKeyframe, one struct with the fields of the calls it replaces: the LK
    settings and Frl of stereo.stereo_match_batch_arrays, the RIGHT camera (a CameraCalibration: model, K, D, iK) with its image size
    and Tcic0_ as priors.stereo_priors and CameraCalibration.computeKeypoints take them, the Frame's ncellsize_ (read without
    rectification), and `tri`, the ov2_tri_params of tri_params() (tri.stereo must be set).  The left camera is the tracker's
    (setCalibration).  The returned struct keeps its distortion array alive."""
    p = L.StereoKeyframeParams()
    p.nklt_win_size, p.nklt_pyr_lvl, p.max_iter = int(nklt_win_size), int(nklt_pyr_lvl), int(nmax_iter)
    p.eps, p.nklt_err, p.fmax_fbklt_dist = float(np.float32(fmax_px_precision)), float(nklt_err), float(fmax_fbklt_dist)
    p.rect = int(bool(rect))
    p.Frl[:] = [0.0] * 9 if Frl is None else [float(v) for v in np.asarray(Frl, np.float64).reshape(9)]
    p.model = right_calib.model
    p.K[:] = [float(v) for v in right_calib.K]
    d = np.zeros(0) if right_calib.D is None else np.ascontiguousarray(right_calib.D, np.float64).reshape(-1)
    p._D = d
    p.D, p.nD = (d.ctypes.data_as(C.POINTER(C.c_double)) if d.size else None), int(d.size)
    p.iK[:] = [float(v) for v in np.asarray(right_calib.iK, np.float64).reshape(9)]
    p.img_w, p.img_h = float(img_w), float(img_h)
    p.Tcic0[:] = [float(v) for v in np.asarray(Tcic0, np.float64).reshape(7)]
    p.ncellsize = int(ncellsize)
    p.tri = _as_params(tri)
    return p


def temporal_keyframe_params(tri, *, n_src_max=16):
    """ov2_temporal_keyframe_params of LockstepTracker.temporalKeyframe: `tri`, the ov2_tri_params of tri_params() as they are
    (tri.stereo is read for the no-motion skip; the stereo fields are not read), and n_src_max, the rows of an item's anchor table:
    the keyframes the keypoints of one keyframe may anchor at (1 .. L.OV2_TKF_MAX_ROWS; fixed by the tracker's first call)."""
    p = L.TemporalKeyframeParams()
    p.tri = _as_params(tri)
    p.n_src_max = int(n_src_max)
    return p


def _as_params(params):
    if isinstance(params, L.TriParams):
        return params
    return tri_params(params["K"], params["iK"], params["Kr"], params["Tlr"], params["Tcic0"], stereo=params["stereo"],
                      rect=params["rect"], fmax_reproj_err=params["fmax_reproj_err"])


def _arr(a, dtype, shape):
    if a is None:
        return None
    a = np.ascontiguousarray(a, dtype=dtype)
    if a.size != int(np.prod(shape)):
        raise ValueError("triangulate: an array has %d elements, %d expected" % (a.size, int(np.prod(shape))))
    return a


def _p(a, ct):
    return a.ctypes.data_as(C.POINTER(ct)) if a is not None else None


def _keyframe(kf):
    """(ov2_tri_keyframe, the arrays it points into, n)"""
    unpx = np.ascontiguousarray(kf["unpx"], np.float32).reshape(-1, 2)
    n = len(unpx)
    src_Twc = kf.get("src_Twc")
    m = 0 if src_Twc is None else int(np.asarray(src_Twc).size // 7)
    keep = dict(Twc=_arr(kf["Twc"], np.float64, (7,)), unpx=unpx, bv=_arr(kf["bv"], np.float64, (n, 3)),
                is_stereo=_arr(kf.get("is_stereo"), np.uint8, (n,)), runpx=_arr(kf.get("runpx"), np.float32, (n, 2)),
                rbv=_arr(kf.get("rbv"), np.float64, (n, 3)), src=_arr(kf.get("src"), np.int32, (n,)),
                src_unpx=_arr(kf.get("src_unpx"), np.float32, (n, 2)), src_bv=_arr(kf.get("src_bv"), np.float64, (n, 3)),
                src_Twc=_arr(src_Twc, np.float64, (m, 7)), src_Tcw=_arr(kf.get("src_Tcw"), np.float64, (m, 7)))
    s = L.TriKeyframe()
    s.n, s.n_src = n, m
    for f in ("Twc", "bv", "rbv", "src_bv", "src_Twc", "src_Tcw"):
        setattr(s, f, _p(keep[f], C.c_double))
    for f in ("unpx", "runpx", "src_unpx"):
        setattr(s, f, _p(keep[f], C.c_float))
    s.is_stereo = _p(keep["is_stereo"], C.c_uint8)
    s.src = _p(keep["src"], C.c_int)
    return s, keep, n


def _result(n):
    out = dict(status=np.zeros(n, np.uint8), wpt=np.zeros((n, 3), np.float64), invdepth=np.zeros(n, np.float64))
    r = L.TriResult()
    r.status = _p(out["status"], C.c_uint8)
    r.wpt = _p(out["wpt"], C.c_double)
    r.invdepth = _p(out["invdepth"], C.c_double)
    return r, out


def _finish(r, out):
    out["counts"] = dict(n_stereo=r.n_stereo, n_stereo_good=r.n_stereo_good, n_candidates=r.n_candidates,
                         n_temporal_good=r.n_temporal_good)
    return out


def triangulate_keyframe(ctx, params, kf):
    """ov2_triangulate_keyframe: both passes for one new keyframe.  Returns a dict with status (n,) uint8 (OV2_TRI_* bits),
    wpt (n,3), invdepth (n,) and counts (the reference's nbstereo / good / candidates / good)."""
    s, keep, n = _keyframe(kf)
    r, out = _result(n)
    L.check(ctx.lib.ov2_triangulate_keyframe(ctx.h, C.byref(_as_params(params)), C.byref(s), C.byref(r)))
    return _finish(r, out)


def triangulate_keyframe_batch(ctx, params, kfs):
    """ov2_triangulate_keyframe_batch: the keyframes of a lock-step batch in one launch (shared params).  Returns one dict per
    keyframe, as triangulate_keyframe."""
    kfs = list(kfs)
    S = (L.TriKeyframe * max(1, len(kfs)))()
    R = (L.TriResult * max(1, len(kfs)))()
    keep, outs = [], []
    for b, kf in enumerate(kfs):
        s, k, n = _keyframe(kf)
        r, out = _result(n)
        S[b], R[b] = s, r
        keep.append(k); outs.append(out)
    L.check(ctx.lib.ov2_triangulate_keyframe_batch(ctx.h, C.byref(_as_params(params)), len(kfs), S, R))
    return [_finish(R[b], outs[b]) for b in range(len(kfs))]


# ---- local-map matching (the plumbing is _mapmatch's, shared with loop_closer.py) ---------------------------------------------------
MATCH_BEHIND, MATCH_OUT_OF_FOV, MATCH_OUT_OF_IMAGE = L.OV2_MATCH_BEHIND, L.OV2_MATCH_OUT_OF_FOV, L.OV2_MATCH_OUT_OF_IMAGE
MATCH_NO_CANDIDATE, MATCH_RATIO_REJECTED, MATCH_BEST = L.OV2_MATCH_NO_CANDIDATE, L.OV2_MATCH_RATIO_REJECTED, L.OV2_MATCH_BEST

_MATCH_FIELDS = (("kp_px", np.float32, C.c_float), ("kp_mp", np.int32, C.c_int), ("cell_start", np.int32, C.c_int),
                 ("cell_kp", np.int32, C.c_int), ("obs_start", np.int32, C.c_int), ("obs_kfid", np.int32, C.c_int),
                 ("obs_kf", np.int32, C.c_int), ("obs_px", np.float32, C.c_float), ("desc_start", np.int32, C.c_int),
                 ("desc", np.uint8, C.c_uint8), ("kf_Tcw", np.float64, C.c_double), ("lm_mp", np.int32, C.c_int),
                 ("lm_wpt", np.float64, C.c_double))
_MATCH = _mapmatch.Family("match_to_map", "ov2_match_to_map", "ov2_match_to_map_batch", L.MatchParams, L.MatchKeyframe, L.MatchResult,
                          _MATCH_FIELDS, scalars=("nb3dkps",))


def match_params(K, D, *, model="pinhole", img_w, img_h, ncellsize, fmax_proj_pxdist, fmax_desc_dist, desc_bytes=32):
    """ov2_match_params: the left camera's model / K (fx fy cx cy) / distortion vector (None or empty: none) / image size, the
    Frame's ncellsize_, and the SlamParams' fmax_proj_pxdist_ and fmax_desc_dist_ as Mapper::matchingToLocalMap passes them.
    The returned struct keeps its distortion array alive."""
    return _MATCH.params(K, D, model, img_w, img_h, ncellsize, fmax_proj_pxdist, fmax_desc_dist, desc_bytes)


_as_match_params = _MATCH.as_params
_match_keyframe = _MATCH.item        # (ov2_match_keyframe, the arrays it points into, n_lm, n_kp)
_match_result = _MATCH.result        # (ov2_match_result, the dict of arrays it points into)


def match_to_map(ctx, params, kf):
    """ov2_match_to_map: Mapper::matchToMap for one keyframe.  Returns a dict with lm_status (n_lm,) uint8 (OV2_MATCH_* bits),
    lm_kp, lm_dist, lm_projpx (n_lm,2), kp_lm (n_kp,) (the winning local-map index per keypoint, -1: none), kp_dist, n_matches."""
    return _MATCH.call(ctx, params, kf)


def match_to_map_batch(ctx, params, kfs):
    """ov2_match_to_map_batch: the keyframes of a lock-step batch in one call (shared params).  Returns one dict per keyframe,
    as match_to_map."""
    return _MATCH.call_batch(ctx, params, kfs)
