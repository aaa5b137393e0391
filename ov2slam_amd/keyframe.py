"""Host-side mirror of the per-frame "frame versus previous keyframe" passes of the reference's src/visual_front_end.cpp on top
of the C ABI (ov2_parallax / ov2_kf_decision / ov2_sampson_filter_2d and their batch forms, csrc/fkf.hip):

    parallax            VisualFrontEnd::computeParallax (:1066-1141) in the arithmetic of each of its three call sites
    kf_decision         VisualFrontEnd::checkNewKfReq (:986-1061)
    sampson_filter_2d   the Sampson pass over the 2-D keypoints after the 5-point search (:610-652)
    epipolar_filter     VisualFrontEnd::epipolar2d2dFiltering (:440-656) as one device chain (ov2_epipolar_filter, csrc/epifilter.hip)
    mono_init           trackMono's un-initialised branch (:98-113) with checkReadyForInit (:855-984) as one device chain
                        (ov2_mono_init, csrc/monoinit.hip)

An item is a dict named like the fields of ov2_fkf_item (the counts follow from the array lengths): cur_lmid (n,), cur_px (n,2),
cur_unpx (n,2), cur_bv (n,3), cur_is3d (n,), cur_Twc (7,), kf_lmid (m,) strictly ascending, kf_unpx (m,2), kf_Tcw (7,), and the
scalars cur_id, kf_id, cur_time, kf_time, kf_nb3dkps, localba_is_on, noccupcells, nb3dkps (-1 or absent: counted on the device).
Poses are [tx ty tz qx qy qz qw], as held by the Frame.  The join by landmark id runs on the device."""
import ctypes as C

import numpy as np

from . import _lib as L

ALL, ONLY_2D, ONLY_3D = L.OV2_FKF_ALL, L.OV2_FKF_ONLY_2D, L.OV2_FKF_ONLY_3D
AVG, MEDIAN, AVG_WIDE = L.OV2_FKF_AVG, L.OV2_FKF_MEDIAN, L.OV2_FKF_AVG_WIDE
EPIF_TOO_FEW_KPS, EPIF_LOW_PARALLAX, EPIF_NO_MODEL, EPIF_DEGENERATE, EPIF_FILTERED = (
    L.OV2_EPIF_TOO_FEW_KPS, L.OV2_EPIF_LOW_PARALLAX, L.OV2_EPIF_NO_MODEL, L.OV2_EPIF_DEGENERATE, L.OV2_EPIF_FILTERED)
(MINIT_RESET, MINIT_LOW_PARALLAX, MINIT_TOO_FEW_KPS, MINIT_TOO_FEW_MATCHES, MINIT_LOW_ROT_PARALLAX, MINIT_NO_MODEL, MINIT_READY,
 MINIT_NOT_REQUESTED, MINIT_NO_KEYFRAME) = (
    L.OV2_MINIT_RESET, L.OV2_MINIT_LOW_PARALLAX, L.OV2_MINIT_TOO_FEW_KPS, L.OV2_MINIT_TOO_FEW_MATCHES, L.OV2_MINIT_LOW_ROT_PARALLAX,
    L.OV2_MINIT_NO_MODEL, L.OV2_MINIT_READY, L.OV2_MINIT_NOT_REQUESTED, L.OV2_MINIT_NO_KEYFRAME)

_FKF_FIELDS = (("cur_lmid", np.int32, C.c_int, 1), ("cur_px", np.float32, C.c_float, 2), ("cur_unpx", np.float32, C.c_float, 2),
               ("cur_bv", np.float64, C.c_double, 3), ("cur_is3d", np.uint8, C.c_uint8, 1), ("kf_lmid", np.int32, C.c_int, 1),
               ("kf_unpx", np.float32, C.c_float, 2))
_FKF_SCALARS = (("cur_id", 0), ("kf_id", 0), ("kf_nb3dkps", 0), ("localba_is_on", 0), ("noccupcells", -1), ("nb3dkps", -1))


def fkf_params(K, *, ncellsize, nbwcells, nbhcells, nbmaxkps, finit_parallax, stereo):
    """ov2_fkf_params: left K (fx fy cx cy), the Frame's grid (ncellsize_, nbwcells_, nbhcells_) and the SlamParams' nbmaxkps_,
    finit_parallax_ and stereo_"""
    p = L.FkfParams()
    p.K[:] = [float(v) for v in np.asarray(K, np.float64).reshape(4)]
    p.ncellsize, p.nbwcells, p.nbhcells, p.nbmaxkps = int(ncellsize), int(nbwcells), int(nbhcells), int(nbmaxkps)
    p.finit_parallax, p.stereo = float(finit_parallax), int(bool(stereo))
    return p


def _as_fkf_params(params):
    if isinstance(params, L.FkfParams):
        return params
    return fkf_params(params["K"], ncellsize=params["ncellsize"], nbwcells=params["nbwcells"], nbhcells=params["nbhcells"],
                      nbmaxkps=params["nbmaxkps"], finit_parallax=params["finit_parallax"], stereo=params["stereo"])


def _fkf_item(item):
    """(ov2_fkf_item, the arrays it points into)"""
    keep = {}
    s = L.FkfItem()
    for name, dt, ct, width in _FKF_FIELDS:
        a = item.get(name)
        a = np.zeros(0, dt) if a is None else np.ascontiguousarray(a, dtype=dt)
        keep[name] = a
        setattr(s, name, a.ctypes.data_as(C.POINTER(ct)))
    s.n_cur, s.n_kf = keep["cur_lmid"].size, keep["kf_lmid"].size
    for name, dt, ct, width in _FKF_FIELDS:
        if keep[name].size != width * (s.n_cur if name.startswith("cur_") else s.n_kf):
            raise ValueError("frame versus keyframe: %s has %d elements, not %d per keypoint" % (name, keep[name].size, width))
    for name in ("cur_Twc", "kf_Tcw"):
        a = np.ascontiguousarray(item.get(name, (0, 0, 0, 0, 0, 0, 1)), np.float64).reshape(7)
        keep[name] = a
        setattr(s, name, a.ctypes.data_as(C.POINTER(C.c_double)))
    for name, default in _FKF_SCALARS:
        setattr(s, name, int(item.get(name, default)))
    s.cur_time, s.kf_time = float(item.get("cur_time", 0.)), float(item.get("kf_time", 0.))
    return s, keep


def _parallax_dict(r):
    return dict(parallax=np.float32(r.parallax), n=r.n, n_distinct=r.n_distinct, n_nonfinite=r.n_nonfinite)


def _decision_dict(r):
    d = _parallax_dict(r)
    d.update(noccupcells=r.noccupcells, nb3dkps=r.nb3dkps, n_out_of_grid=r.n_out_of_grid, decision=r.decision, reason=r.reason)
    return d


def _items(items):
    items = list(items)
    S = (L.FkfItem * max(1, len(items)))()
    keep = []
    for b, it in enumerate(items):
        S[b], k = _fkf_item(it)
        keep.append(k)
    return items, S, keep


def parallax(ctx, params, item, *, unrot, filter=ALL, stat=AVG):
    """ov2_parallax: computeParallax(kfid, do_unrot, bmedian, b2donly) is (unrot, ONLY_2D if b2donly else ALL, MEDIAN if bmedian
    else AVG); the gate ahead of the 5-point search is (1, ONLY_3D if epifrom3dkps else ALL, AVG_WIDE).  Returns a dict with
    parallax (np.float32), n, n_distinct, n_nonfinite."""
    s, keep = _fkf_item(item)
    r = L.ParallaxResult()
    L.check(ctx.lib.ov2_parallax(ctx.h, C.byref(_as_fkf_params(params)), C.byref(s), int(unrot), int(filter), int(stat), C.byref(r)))
    return _parallax_dict(r)


def parallax_batch(ctx, params, items, *, unrot, filter=ALL, stat=AVG):
    """ov2_parallax_batch: the frames of a lock-step batch in one launch (shared params and form); one dict per item"""
    items, S, keep = _items(items)
    R = (L.ParallaxResult * max(1, len(items)))()
    L.check(ctx.lib.ov2_parallax_batch(ctx.h, C.byref(_as_fkf_params(params)), len(items), S, int(unrot), int(filter), int(stat), R))
    return [_parallax_dict(R[b]) for b in range(len(items))]


def kf_decision(ctx, params, item):
    """ov2_kf_decision: checkNewKfReq.  Returns the parallax fields plus noccupcells, nb3dkps (as used by the rule), n_out_of_grid,
    decision (0 / 1) and reason (OV2_KF_* bits)."""
    s, keep = _fkf_item(item)
    r = L.KfDecisionResult()
    L.check(ctx.lib.ov2_kf_decision(ctx.h, C.byref(_as_fkf_params(params)), C.byref(s), C.byref(r)))
    return _decision_dict(r)


def kf_decision_batch(ctx, params, items):
    """ov2_kf_decision_batch: one small record per item comes back; one dict per item"""
    items, S, keep = _items(items)
    R = (L.KfDecisionResult * max(1, len(items)))()
    L.check(ctx.lib.ov2_kf_decision_batch(ctx.h, C.byref(_as_fkf_params(params)), len(items), S, R))
    return [_decision_dict(R[b]) for b in range(len(items))]


def _sampson_result(n):
    out = dict(err=np.zeros(n, np.float32), bad=np.zeros(n, np.uint8))
    r = L.Sampson2dResult()
    r.err, r.bad = out["err"].ctypes.data_as(C.POINTER(C.c_float)), out["bad"].ctypes.data_as(C.POINTER(C.c_uint8))
    return r, out


def sampson_filter_2d(ctx, item, Fkfcur, fransac_err):
    """ov2_sampson_filter_2d: err (n,) float32 and bad (n,) uint8 per current keypoint (0 for 3-D keypoints), n_bad.  A 2-D
    keypoint the keyframe does not hold is scored against (0, 0), as the reference does."""
    s, keep = _fkf_item(item)
    r, out = _sampson_result(s.n_cur)
    F = np.ascontiguousarray(Fkfcur, np.float64).reshape(9)
    L.check(ctx.lib.ov2_sampson_filter_2d(ctx.h, C.byref(s), F.ctypes.data_as(C.POINTER(C.c_double)), float(fransac_err), C.byref(r)))
    out["n_bad"] = r.n_bad
    return out


def sampson_filter_2d_batch(ctx, items, Fkfcur, fransac_err):
    """ov2_sampson_filter_2d_batch: Fkfcur is (n_items, 9); one dict per item"""
    items, S, keep = _items(items)
    F = np.ascontiguousarray(Fkfcur, np.float64).reshape(len(items), 9)
    R = (L.Sampson2dResult * max(1, len(items)))()
    outs = []
    for b in range(len(items)):
        R[b], out = _sampson_result(S[b].n_cur)
        outs.append(out)
    L.check(ctx.lib.ov2_sampson_filter_2d_batch(ctx.h, len(items), S, F.ctypes.data_as(C.POINTER(C.c_double)), float(fransac_err), R))
    for b, out in enumerate(outs):
        out["n_bad"] = R[b].n_bad
    return outs


def se3_inverse(T):
    """ov2_se3_inverse: [t q] of the inverse of the transform [t q] in the library's host arithmetic -- the kf_Tcw that
    LockstepTracker.setKeyframe derives from kf_Twc, bit for bit"""
    T = np.ascontiguousarray(T, np.float64).reshape(7)
    out = np.zeros(7, np.float64)
    L.check(L.load().ov2_se3_inverse(T.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)))
    return out


# ---- epipolar2d2dFiltering ----------------------------------------------------------------------------------------------------------
def epifilter_params(fkf, *, max_iterations, threshold, fransac_err, mono, n_rows, probability=0.99, boptimize=False):
    """ov2_epifilter_params: the ov2_fkf_params (or the dict of them; K and stereo are read), the search's nransac_iter_ and bearing
    threshold, SlamParams::fransac_err_ (pixels) and mono_, and the rows of the sample table drawn per item"""
    p = L.EpifilterParams()
    p.fkf = _as_fkf_params(fkf)
    p.epi.max_iterations, p.epi.threshold, p.epi.probability = int(max_iterations), float(threshold), float(probability)
    p.epi.boptimize = int(bool(boptimize))
    p.fransac_err, p.mono, p.n_rows = float(fransac_err), int(bool(mono)), int(n_rows)
    return p


def _as_epifilter_params(params):
    if isinstance(params, L.EpifilterParams):
        return params
    return epifilter_params(params["fkf"], max_iterations=params["max_iterations"], threshold=params["threshold"],
                            fransac_err=params["fransac_err"], mono=params["mono"], n_rows=params["n_rows"],
                            probability=params.get("probability", 0.99), boptimize=params.get("boptimize", False))


def _epifilter_item(item):
    """(ov2_epifilter_item, the arrays it points into): the ov2_fkf_item dict plus kf_bv (m, 3), kf_Twc (7,), nbkfs, seed"""
    s = L.EpifilterItem()
    s.fkf, keep = _fkf_item(item)
    a = item.get("kf_bv")
    a = np.zeros(0, np.float64) if a is None else np.ascontiguousarray(a, np.float64)
    if a.size != 3 * s.fkf.n_kf:
        raise ValueError("frame versus keyframe: kf_bv has %d elements, not 3 per keypoint" % a.size)
    keep["kf_bv"] = a
    keep["kf_Twc"] = np.ascontiguousarray(item.get("kf_Twc", (0, 0, 0, 0, 0, 0, 1)), np.float64).reshape(7)
    s.kf_bv, s.kf_Twc = (keep[k].ctypes.data_as(C.POINTER(C.c_double)) for k in ("kf_bv", "kf_Twc"))
    s.nbkfs, s.seed = int(item.get("nbkfs", 0)), int(item.get("seed", 0)) & ((1 << 64) - 1)
    return s, keep


def _epifilter_result(n, n_rows, trace):
    out = dict(removed=np.zeros(n, np.uint8), pair_cur=np.zeros(n, np.int32), err=np.zeros(n, np.float32))
    r = L.EpifilterResult()
    r.removed = out["removed"].ctypes.data_as(C.POINTER(C.c_uint8))
    r.pair_cur = out["pair_cur"].ctypes.data_as(C.POINTER(C.c_int))
    r.err = out["err"].ctypes.data_as(C.POINTER(C.c_float))
    if trace:
        out["samples"] = np.full((n_rows, 8), -1, np.int32)
        r.trace_samples = out["samples"].ctypes.data_as(C.POINTER(C.c_int))
    return r, out


def _epifilter_dict(r, out):
    out.update(action=r.action, m=r.m, epifrom3dkps=r.epifrom3dkps, do_optimize=r.do_optimize, nb3dkps=r.nb3dkps,
               parallax=np.float32(r.parallax), status=r.status, best_row=r.best_row, iterations=r.iterations,
               rows_consumed=r.rows_consumed, score=np.float64(r.score), n_inliers=r.n_inliers, n_outliers=r.n_outliers,
               model=np.array(r.model[:], np.float64), F=np.array(r.F[:], np.float64), n_removed_ransac=r.n_removed_ransac,
               n_removed_sampson=r.n_removed_sampson, pose_from_model=r.pose_from_model, Twc_model=np.array(r.Twc_model[:], np.float64))
    out["pair_cur"] = out["pair_cur"][:max(r.m, 0)]
    if "samples" in out and not (r.action >= EPIF_NO_MODEL and r.m >= 8):
        out["samples"] = None                                      # no table was drawn
    return out


def epipolar_filter(ctx, params, item, *, trace_samples=False):
    """ov2_epipolar_filter: epipolar2d2dFiltering of one frame.  Returns a dict named like ov2_epifilter_result: action (EPIF_*), m,
    epifrom3dkps, do_optimize, nb3dkps, parallax (np.float32), the search's status / best_row / iterations / rows_consumed / score /
    n_inliers / n_outliers / model (12,), F (9,), n_removed_ransac, n_removed_sampson, removed (n,) uint8 (0 kept, 1 RANSAC outlier,
    2 Sampson pass), pair_cur (m,), err (n,) float32, pose_from_model, Twc_model (7,); with trace_samples the table the device drew
    (n_rows, 8), None where the item did not search."""
    p = _as_epifilter_params(params)
    s, keep = _epifilter_item(item)
    r, out = _epifilter_result(s.fkf.n_cur, p.n_rows, trace_samples)
    L.check(ctx.lib.ov2_epipolar_filter(ctx.h, C.byref(p), C.byref(s), C.byref(r)))
    return _epifilter_dict(r, out)


def epipolar_filter_batch(ctx, params, items, *, trace_samples=False):
    """ov2_epipolar_filter_batch: the frames of a lock-step batch in one chain (shared params); one dict per item"""
    p = _as_epifilter_params(params)
    items = list(items)
    S = (L.EpifilterItem * max(1, len(items)))()
    R = (L.EpifilterResult * max(1, len(items)))()
    keep, outs = [], []
    for b, it in enumerate(items):
        S[b], k = _epifilter_item(it)
        R[b], out = _epifilter_result(S[b].fkf.n_cur, p.n_rows, trace_samples)
        keep.append(k)
        outs.append(out)
    L.check(ctx.lib.ov2_epipolar_filter_batch(ctx.h, C.byref(p), len(items), S, R))
    return [_epifilter_dict(R[b], outs[b]) for b in range(len(items))]


# ---- mono initialisation ------------------------------------------------------------------------------------------------------------
def mono_init_params(fkf, *, max_iterations, threshold, n_rows, min_2d_kps=50, probability=0.99, boptimize=False):
    """ov2_mono_init_params: the ov2_fkf_params (or the dict of them; K and finit_parallax are read), the search's nransac_iter_ and
    bearing threshold, the rows of the sample table drawn per item and the 2-D keypoint count below which trackMono asks for a reset
    (the reference's literal 50; 0: no such test)"""
    p = L.MonoInitParams()
    p.fkf = _as_fkf_params(fkf)
    p.epi.max_iterations, p.epi.threshold, p.epi.probability = int(max_iterations), float(threshold), float(probability)
    p.epi.boptimize = int(bool(boptimize))
    p.n_rows, p.min_2d_kps = int(n_rows), int(min_2d_kps)
    return p


def _as_mono_init_params(params):
    if isinstance(params, L.MonoInitParams):
        return params
    return mono_init_params(params["fkf"], max_iterations=params["max_iterations"], threshold=params["threshold"],
                            n_rows=params["n_rows"], min_2d_kps=params.get("min_2d_kps", 50),
                            probability=params.get("probability", 0.99), boptimize=params.get("boptimize", False))


def _mono_init_item(item):
    """(ov2_mono_init_item, the arrays it points into): the ov2_fkf_item dict plus kf_bv (m, 3) and seed"""
    s = L.MonoInitItem()
    s.fkf, keep = _fkf_item(item)
    a = item.get("kf_bv")
    a = np.zeros(0, np.float64) if a is None else np.ascontiguousarray(a, np.float64)
    if a.size != 3 * s.fkf.n_kf:
        raise ValueError("frame versus keyframe: kf_bv has %d elements, not 3 per keypoint" % a.size)
    keep["kf_bv"] = a
    s.kf_bv = a.ctypes.data_as(C.POINTER(C.c_double))
    s.seed = int(item.get("seed", 0)) & ((1 << 64) - 1)
    return s, keep


def _mono_init_result(n, n_rows, trace):
    out = dict(removed=np.zeros(n, np.uint8), pair_cur=np.zeros(n, np.int32))
    r = L.MonoInitResult()
    r.removed = out["removed"].ctypes.data_as(C.POINTER(C.c_uint8))
    r.pair_cur = out["pair_cur"].ctypes.data_as(C.POINTER(C.c_int))
    if trace:
        out["samples"] = np.full((n_rows, 8), -1, np.int32)
        r.trace_samples = out["samples"].ctypes.data_as(C.POINTER(C.c_int))
    return r, out


def _mono_init_record(r):
    """the scalar and fixed-size fields of an ov2_mono_init_result"""
    return _mono_init_fields(r, {})


def _mono_init_dict(r, out):
    _mono_init_fields(r, out)
    out["pair_cur"] = out["pair_cur"][:max(r.m, 0)]
    if "samples" in out and not (MINIT_NO_MODEL <= r.action <= MINIT_READY and out["samples"].shape[0] > 0):
        out["samples"] = None                                      # no table was drawn
    return out


def _mono_init_fields(r, out):
    out.update(action=r.action, nb2dkps=r.nb2dkps, p0=np.float32(r.p0), p0_n=r.p0_n, p0_n_distinct=r.p0_n_distinct,
               p0_n_nonfinite=r.p0_n_nonfinite, m=r.m, p1=np.float32(r.p1), status=r.status, best_row=r.best_row,
               iterations=r.iterations, rows_consumed=r.rows_consumed, score=np.float64(r.score), n_inliers=r.n_inliers,
               n_outliers=r.n_outliers, model=np.array(r.model[:], np.float64), n_removed=r.n_removed, pose_refined=r.pose_refined,
               Twc_init=np.array(r.Twc_init[:], np.float64))
    return out


def mono_init(ctx, params, item, *, trace_samples=False):
    """ov2_mono_init: the mono initialisation test of one frame against its keyframe.  Returns a dict named like
    ov2_mono_init_result: action (MINIT_*), nb2dkps, p0 (np.float32) with p0_n / p0_n_distinct / p0_n_nonfinite, m, p1 (np.float32),
    the search's status / best_row / iterations / rows_consumed / score / n_inliers / n_outliers / model (12,), n_removed, removed
    (n,) uint8, pair_cur (m,), Twc_init (7,) -- the pose of the UNREFINED model, pose_refined = 0 --; with trace_samples the table
    the device drew (n_rows, 8), None where the item did not search."""
    p = _as_mono_init_params(params)
    s, keep = _mono_init_item(item)
    r, out = _mono_init_result(s.fkf.n_cur, p.n_rows, trace_samples)
    L.check(ctx.lib.ov2_mono_init(ctx.h, C.byref(p), C.byref(s), C.byref(r)))
    return _mono_init_dict(r, out)


def mono_init_batch(ctx, params, items, *, trace_samples=False):
    """ov2_mono_init_batch: the frames of a lock-step batch in one chain (shared params); one dict per item"""
    p = _as_mono_init_params(params)
    items = list(items)
    S = (L.MonoInitItem * max(1, len(items)))()
    R = (L.MonoInitResult * max(1, len(items)))()
    keep, outs = [], []
    for b, it in enumerate(items):
        S[b], k = _mono_init_item(it)
        R[b], out = _mono_init_result(S[b].fkf.n_cur, p.n_rows, trace_samples)
        keep.append(k)
        outs.append(out)
    L.check(ctx.lib.ov2_mono_init_batch(ctx.h, C.byref(p), len(items), S, R))
    return [_mono_init_dict(R[b], outs[b]) for b in range(len(items))]
