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
Poses are [tx ty tz qx qy qz qw], as held by the Frame."""
import ctypes as C

import numpy as np

from . import _lib as L

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
