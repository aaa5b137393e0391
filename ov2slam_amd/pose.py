"""Host-side mirror of the absolute-pose search (the reference's MultiViewGeometry::p3pRansac with USE_OPENGV,
src/multi_view_geometry.cpp:144-343) on top of the C ABI (ov2_p3p_ransac[_batch], csrc/p3p.hip): Kneip's P3P hypotheses from a
sample table that is an input, searched as OpenGV's LMedS or RANSAC loop would, so that a call is a deterministic function of its
arguments.  draw_samples() fills a table (ov2_p3p_draw_samples, host only).

A problem is a dict: bv (n,3) unit bearing vectors in the camera frame, X (n,3) world points, samples (rows,4) int32.
OpenGV's non-linear refinement (boptimize) is not provided: refine the returned pose with MultiViewGeometry.ceresPnP, as
LoopCloser::computePnP does right after."""
import ctypes as C
import math

import numpy as np

from . import _lib as L

LMEDS, RANSAC = L.OV2_P3P_LMEDS, L.OV2_P3P_RANSAC
TOO_FEW_POINTS, NO_MODEL = L.OV2_P3P_TOO_FEW_POINTS, L.OV2_P3P_NO_MODEL
FEW_INLIERS, NOT_ORTHOGONAL = L.OV2_P3P_FEW_INLIERS, L.OV2_P3P_NOT_ORTHOGONAL
MAX_POINTS, MAX_ROWS = L.OV2_P3P_MAX_POINTS, L.OV2_P3P_MAX_ROWS


def threshold(errth, fx, fy):
    """the reference's 1 - cos(atan(errth / focal)): focal is the float (fx + fy) / 2, the quotient a float, cos / atan in double"""
    focal = np.float32(np.float32(fx) + np.float32(fy))
    focal = np.float32(np.float64(focal) / 2.)
    return 1.0 - math.cos(math.atan(float(np.float32(errth) / focal)))


def draw_samples(seed, n, rows):
    """ov2_p3p_draw_samples: (rows, 4) int32, four distinct indices of [0, n) per row"""
    out = np.zeros((max(int(rows), 0), 4), np.int32)
    L.check(L.load().ov2_p3p_draw_samples(int(seed) & 0xFFFFFFFFFFFFFFFF, int(n), int(rows), out.ctypes.data_as(C.POINTER(C.c_int))))
    return out


def p3p_params(mode, max_iterations, threshold, probability=0.99, boptimize=False):
    p = L.P3PParams()
    p.mode, p.max_iterations, p.threshold, p.probability, p.boptimize = int(mode), int(max_iterations), float(threshold), float(probability), int(bool(boptimize))
    return p


def _as_params(params):
    if isinstance(params, L.P3PParams):
        return params
    return p3p_params(params["mode"], params["max_iterations"], params["threshold"], params.get("probability", 0.99),
                      params.get("boptimize", False))


def _problem(pb, trace):
    """(ov2_p3p_problem, ov2_p3p_result, the arrays they point into)"""
    bv = np.ascontiguousarray(pb["bv"], np.float64).reshape(-1, 3)
    X = np.ascontiguousarray(pb["X"], np.float64).reshape(-1, 3)
    sm = np.ascontiguousarray(pb["samples"], np.int32).reshape(-1, 4)
    if len(bv) != len(X):
        raise ValueError("p3p_ransac: %d bearing vectors, %d world points" % (len(bv), len(X)))
    n, S = len(bv), len(sm)
    keep = dict(bv=bv, X=X, samples=sm, outliers=np.zeros(max(n, 1), np.int32))
    s = L.P3PProblem()
    s.n, s.n_rows = n, S
    s.bv = bv.ctypes.data_as(C.POINTER(C.c_double)) if n else None
    s.X = X.ctypes.data_as(C.POINTER(C.c_double)) if n else None
    s.samples = sm.ctypes.data_as(C.POINTER(C.c_int)) if S else None
    r = L.P3PResult()
    r.outliers = keep["outliers"].ctypes.data_as(C.POINTER(C.c_int))
    if trace:
        keep["trace_valid"], keep["trace_score"] = np.zeros(max(S, 1), np.uint8), np.zeros(max(S, 1), np.float64)
        r.trace_valid = keep["trace_valid"].ctypes.data_as(C.POINTER(C.c_uint8))
        r.trace_score = keep["trace_score"].ctypes.data_as(C.POINTER(C.c_double))
    return s, r, keep


def _finish(r, keep, trace):
    S = len(keep["samples"])
    out = dict(model=np.array(r.model[:], np.float64), score=r.score, best_row=r.best_row, iterations=r.iterations,
               rows_consumed=r.rows_consumed, status=r.status, n_inliers=r.n_inliers,
               outliers=keep["outliers"][:r.n_outliers].copy(), ok=r.status == 0)
    out["Rwc"], out["twc"] = out["model"][:9].reshape(3, 3), out["model"][9:]
    if trace:
        out["trace_valid"], out["trace_score"] = keep["trace_valid"][:S], keep["trace_score"][:S]
    return out


def p3p_ransac(ctx, params, problem, trace=False):
    """ov2_p3p_ransac.  Returns a dict: model (12,) (Rwc row-major, twc; also as Rwc (3,3) and twc (3,)), score, best_row,
    iterations, rows_consumed, status (OV2_P3P_* bits), ok (status == 0: the reference returns true), n_inliers, outliers
    (ascending int32) and, with trace, trace_valid / trace_score per row."""
    s, r, keep = _problem(problem, trace)
    L.check(ctx.lib.ov2_p3p_ransac(ctx.h, C.byref(_as_params(params)), C.byref(s), C.byref(r)))
    return _finish(r, keep, trace)


def p3p_ransac_batch(ctx, params, problems, trace=False):
    """ov2_p3p_ransac_batch: the problems of a lock-step batch in one call (shared params, sizes may differ).  Returns one dict
    per problem, as p3p_ransac."""
    problems = list(problems)
    S = (L.P3PProblem * max(1, len(problems)))()
    R = (L.P3PResult * max(1, len(problems)))()
    keeps = []
    for b, pb in enumerate(problems):
        S[b], R[b], k = _problem(pb, trace)
        keeps.append(k)
    L.check(ctx.lib.ov2_p3p_ransac_batch(ctx.h, C.byref(_as_params(params)), len(problems), S, R))
    return [_finish(R[b], keeps[b], trace) for b in range(len(problems))]


# ---- relative pose: the five-point essential-matrix search (ov2_epipolar_ransac[_batch], csrc/fivept.hip) --------------------------
# The reference's MultiViewGeometry::compute5ptEssentialMatrix with USE_OPENGV (src/multi_view_geometry.cpp:594-696): Nister's solver
# under OpenGV's RANSAC loop, restated (tests/fivept_ref.py), not pinned against an OpenGV binary.  A problem is a dict: bv1 (n,3)
# unit bearings of the keyframe, bv2 (n,3) of the current frame, samples (rows,8) int32.  The model is x1 = R x2 + t (Rwc, twc).
EPI_TOO_FEW_POINTS, EPI_NO_MODEL, EPI_FEW_INLIERS = L.OV2_EPI_TOO_FEW_POINTS, L.OV2_EPI_NO_MODEL, L.OV2_EPI_FEW_INLIERS
EPI_MAX_POINTS, EPI_MAX_ROWS = L.OV2_EPI_MAX_POINTS, L.OV2_EPI_MAX_ROWS


def epipolar_threshold(errth, fx, fy):
    """the reference's 2 (1 - cos(atan(errth / focal))): focal is the float (fx + fy) / 2, the quotient a float, cos / atan in double"""
    return 2.0 * threshold(errth, fx, fy)


def epipolar_draw_samples(seed, n, rows):
    """ov2_epipolar_draw_samples: (rows, 8) int32, eight distinct indices of [0, n) per row"""
    out = np.zeros((max(int(rows), 0), 8), np.int32)
    L.check(L.load().ov2_epipolar_draw_samples(int(seed) & 0xFFFFFFFFFFFFFFFF, int(n), int(rows), out.ctypes.data_as(C.POINTER(C.c_int))))
    return out


def epipolar_params(max_iterations, threshold, probability=0.99, boptimize=False):
    p = L.EpipolarParams()
    p.max_iterations, p.threshold, p.probability, p.boptimize = int(max_iterations), float(threshold), float(probability), int(bool(boptimize))
    return p


def _epi_as_params(params):
    if isinstance(params, L.EpipolarParams):
        return params
    return epipolar_params(params["max_iterations"], params["threshold"], params.get("probability", 0.99), params.get("boptimize", False))


def _epi_problem(pb, trace):
    """(ov2_epipolar_problem, ov2_epipolar_result, the arrays they point into)"""
    bv1 = np.ascontiguousarray(pb["bv1"], np.float64).reshape(-1, 3)
    bv2 = np.ascontiguousarray(pb["bv2"], np.float64).reshape(-1, 3)
    sm = np.ascontiguousarray(pb["samples"], np.int32).reshape(-1, 8)
    if len(bv1) != len(bv2):
        raise ValueError("epipolar_ransac: %d and %d bearing vectors" % (len(bv1), len(bv2)))
    n, S = len(bv1), len(sm)
    keep = dict(bv1=bv1, bv2=bv2, samples=sm, outliers=np.zeros(max(n, 1), np.int32))
    s = L.EpipolarProblem()
    s.n, s.n_rows = n, S
    s.bv1 = bv1.ctypes.data_as(C.POINTER(C.c_double)) if n else None
    s.bv2 = bv2.ctypes.data_as(C.POINTER(C.c_double)) if n else None
    s.samples = sm.ctypes.data_as(C.POINTER(C.c_int)) if S else None
    r = L.EpipolarResult()
    r.outliers = keep["outliers"].ctypes.data_as(C.POINTER(C.c_int))
    if trace:
        keep["trace_valid"], keep["trace_score"] = np.zeros(max(S, 1), np.uint8), np.zeros(max(S, 1), np.float64)
        keep["trace_model"] = np.zeros((max(S, 1), 12), np.float64)
        r.trace_valid = keep["trace_valid"].ctypes.data_as(C.POINTER(C.c_uint8))
        r.trace_score = keep["trace_score"].ctypes.data_as(C.POINTER(C.c_double))
        r.trace_model = keep["trace_model"].ctypes.data_as(C.POINTER(C.c_double))
    return s, r, keep


def _epi_finish(r, keep, trace):
    S = len(keep["samples"])
    out = dict(model=np.array(r.model[:], np.float64), score=r.score, best_row=r.best_row, iterations=r.iterations,
               rows_consumed=r.rows_consumed, status=r.status, n_inliers=r.n_inliers,
               outliers=keep["outliers"][:r.n_outliers].copy(), ok=r.status == 0)
    out["Rwc"], out["twc"] = out["model"][:9].reshape(3, 3), out["model"][9:]
    if trace:
        out["trace_valid"], out["trace_score"], out["trace_model"] = keep["trace_valid"][:S], keep["trace_score"][:S], keep["trace_model"][:S]
    return out


def epipolar_ransac(ctx, params, problem, trace=False):
    """ov2_epipolar_ransac.  Returns a dict: model (12,) (R row-major, t; also as Rwc (3,3) and twc (3,)), score, best_row,
    iterations, rows_consumed, status (OV2_EPI_* bits), ok (status == 0: the reference returns true), n_inliers, outliers
    (ascending int32) and, with trace, trace_valid / trace_score / trace_model per row."""
    s, r, keep = _epi_problem(problem, trace)
    L.check(ctx.lib.ov2_epipolar_ransac(ctx.h, C.byref(_epi_as_params(params)), C.byref(s), C.byref(r)))
    return _epi_finish(r, keep, trace)


def epipolar_ransac_batch(ctx, params, problems, trace=False):
    """ov2_epipolar_ransac_batch: the problems of a lock-step batch in one call (shared params, sizes may differ).  Returns one
    dict per problem, as epipolar_ransac."""
    problems = list(problems)
    S = (L.EpipolarProblem * max(1, len(problems)))()
    R = (L.EpipolarResult * max(1, len(problems)))()
    keeps = []
    for b, pb in enumerate(problems):
        S[b], R[b], k = _epi_problem(pb, trace)
        keeps.append(k)
    L.check(ctx.lib.ov2_epipolar_ransac_batch(ctx.h, C.byref(_epi_as_params(params)), len(problems), S, R))
    return [_epi_finish(R[b], keeps[b], trace) for b in range(len(problems))]
