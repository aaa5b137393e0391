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


# ---- the per-frame pose (f15): ceresPnP in one launch and computePose as one device-resident chain (csrc/pnp.hip) -----------------
# MultiViewGeometry::ceresPnP (src/multi_view_geometry.cpp:492-586) and VisualFrontEnd::computePose (src/visual_front_end.cpp:659-851).
# A PnP problem is a dict: unpx (n,2) undistorted pixels, wpt (n,3) world points, scale (n,) int pyramid levels (sigma = 2^scale;
# omitted: zeros), Twc (7,) [t q(xyzw)].  A pose problem adds bv (n,3), do_p3p, p3p_req and samples (rows,4) (read only where do_p3p).
TOO_FEW, POSE_OK, PNP_REQ_P3P = L.OV2_POSE_TOO_FEW, L.OV2_POSE_OK, L.OV2_POSE_PNP_REQ_P3P
P3P_RESET, PNP_RESET, PNP_KEEP = L.OV2_POSE_P3P_RESET, L.OV2_POSE_PNP_RESET, L.OV2_POSE_PNP_KEEP
ACTION_NAMES = {TOO_FEW: "TOO_FEW", POSE_OK: "POSE_OK", PNP_REQ_P3P: "PNP_REQ_P3P", P3P_RESET: "P3P_RESET", PNP_RESET: "PNP_RESET",
                PNP_KEEP: "PNP_KEEP"}


def pnp_params(nmaxiter, chi2th, use_robust, apply_l2_after_robust, K):
    p = L.PnPParams()
    p.nmaxiter, p.chi2th, p.use_robust, p.apply_l2_after_robust = int(nmaxiter), float(chi2th), int(bool(use_robust)), int(bool(apply_l2_after_robust))
    p.K[:] = [float(v) for v in K]
    return p


def _as_pnp_params(params):
    if isinstance(params, L.PnPParams):
        return params
    return pnp_params(params.get("nmaxiter", 5), params["chi2th"], params.get("use_robust", True),
                      params.get("apply_l2_after_robust", True), params["K"])


def pose_params(pnp, p3p, mono):
    p = L.PoseParams()
    p.pnp, p.p3p, p.mono = _as_pnp_params(pnp), _as_params(p3p), int(bool(mono))
    return p


def _as_pose_params(params):
    if isinstance(params, L.PoseParams):
        return params
    return pose_params(params["pnp"], params["p3p"], params.get("mono", False))


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _pnp_arrays(pb, who):
    unpx = np.ascontiguousarray(pb["unpx"], np.float64).reshape(-1, 2)
    wpt = np.ascontiguousarray(pb["wpt"], np.float64).reshape(-1, 3)
    n = len(unpx)
    scale = np.ascontiguousarray(pb["scale"] if pb.get("scale") is not None else np.zeros(n), np.int32).reshape(-1)
    Twc = np.ascontiguousarray(pb["Twc"], np.float64).reshape(-1)
    if len(wpt) != n or len(scale) != n or len(Twc) != 7:
        raise ValueError("%s: %d pixels, %d world points, %d scales, %d pose entries" % (who, n, len(wpt), len(scale), len(Twc)))
    return n, unpx, wpt, scale, Twc


def _passes(r):
    return [dict(ran=bool(q.ran), iterations=q.iterations, num_successful_steps=q.num_successful_steps, termination=q.termination,
                 initial_cost=q.initial_cost, final_cost=q.final_cost) for q in r.passes]


def _pnp_problem(pb):
    n, unpx, wpt, scale, Twc = _pnp_arrays(pb, "ceres_pnp")
    keep = dict(unpx=unpx, wpt=wpt, scale=scale, Twc=Twc, outliers=np.zeros(max(n, 1), np.int32))
    s = L.PnPProblem()
    s.n, s.Twc = n, _dp(Twc)
    s.unpx, s.wpt = (_dp(unpx), _dp(wpt)) if n else (None, None)
    s.scale = scale.ctypes.data_as(C.POINTER(C.c_int)) if n else None
    r = L.PnPResult()
    r.outliers = keep["outliers"].ctypes.data_as(C.POINTER(C.c_int))
    return s, r, keep


def _pnp_finish(r, keep):
    return dict(success=bool(r.success), Twc=np.array(r.Twc[:], np.float64), outliers=keep["outliers"][:r.n_outliers].copy(),
                passes=_passes(r))


def ceres_pnp(ctx, params, problem):
    """ov2_ceres_pnp: the two-pass protocol of ceresPnP in one launch.  Returns a dict: success, Twc (7,), outliers (ascending int32,
    the first test's) and passes (two dicts: ran, iterations, num_successful_steps, termination, initial_cost, final_cost)."""
    s, r, keep = _pnp_problem(problem)
    L.check(ctx.lib.ov2_ceres_pnp(ctx.h, C.byref(_as_pnp_params(params)), C.byref(s), C.byref(r)))
    return _pnp_finish(r, keep)


def ceres_pnp_batch(ctx, params, problems):
    """ov2_ceres_pnp_batch: the problems of a lock-step batch in one launch (shared params, sizes may differ); one dict per problem,
    bit for bit what ceres_pnp gives on it."""
    problems = list(problems)
    S = (L.PnPProblem * max(1, len(problems)))()
    R = (L.PnPResult * max(1, len(problems)))()
    keeps = []
    for b, pb in enumerate(problems):
        S[b], R[b], k = _pnp_problem(pb)
        keeps.append(k)
    L.check(ctx.lib.ov2_ceres_pnp_batch(ctx.h, C.byref(_as_pnp_params(params)), len(problems), S, R))
    return [_pnp_finish(R[b], keeps[b]) for b in range(len(problems))]


def _pose_problem(pb):
    n, unpx, wpt, scale, Twc = _pnp_arrays(pb, "compute_pose")
    do_p3p = bool(pb.get("do_p3p", False))
    keep = dict(unpx=unpx, wpt=wpt, scale=scale, Twc=Twc, removed=np.zeros(max(n, 1), np.uint8))
    s = L.PoseProblem()
    s.n, s.Twc, s.do_p3p, s.p3p_req = n, _dp(Twc), int(do_p3p), int(bool(pb.get("p3p_req", False)))
    s.unpx, s.wpt = (_dp(unpx), _dp(wpt)) if n else (None, None)
    s.scale = scale.ctypes.data_as(C.POINTER(C.c_int)) if n else None
    if do_p3p:
        bv = np.ascontiguousarray(pb["bv"], np.float64).reshape(-1, 3)
        sm = np.ascontiguousarray(pb["samples"], np.int32).reshape(-1, 4)
        if len(bv) != n:
            raise ValueError("compute_pose: %d bearing vectors, %d keypoints" % (len(bv), n))
        keep["bv"], keep["samples"] = bv, sm
        s.bv = _dp(bv) if n else None
        s.n_rows = len(sm)
        s.samples = sm.ctypes.data_as(C.POINTER(C.c_int)) if len(sm) else None
    r = L.PoseResult()
    r.removed = keep["removed"].ctypes.data_as(C.POINTER(C.c_uint8))
    return s, r, keep


def _pose_finish(r, keep):
    n = len(keep["unpx"])
    return dict(Twc=np.array(r.Twc[:], np.float64), action=r.action, p3p_req_out=bool(r.p3p_req_out), removed=keep["removed"][:n].copy(),
                n_removed_p3p=r.n_removed_p3p, n_outliers_pnp=r.n_outliers_pnp, ran_p3p=bool(r.ran_p3p),
                p3p=dict(status=r.p3p_status, best_row=r.p3p_best_row, iterations=r.p3p_iterations, rows_consumed=r.p3p_rows_consumed,
                         score=r.p3p_score), passes=_passes(r))


def compute_pose(ctx, params, problem):
    """ov2_compute_pose: VisualFrontEnd::computePose as one device-resident chain (P3P -> compaction -> ceresPnP -> decision), one
    synchronisation.  Returns a dict: Twc (7,), action (OV2_POSE_*), p3p_req_out, removed (n,) uint8 (0 kept, 1 after P3P, 2 after an
    accepted PnP), n_removed_p3p, n_outliers_pnp, ran_p3p, p3p (status, best_row, iterations, rows_consumed, score), passes."""
    s, r, keep = _pose_problem(problem)
    L.check(ctx.lib.ov2_compute_pose(ctx.h, C.byref(_as_pose_params(params)), C.byref(s), C.byref(r)))
    return _pose_finish(r, keep)


def compute_pose_batch(ctx, params, problems):
    """ov2_compute_pose_batch: the frames of a lock-step batch in one call (shared params, sizes and do_p3p may differ); one dict
    per frame, bit for bit what compute_pose gives on it."""
    problems = list(problems)
    S = (L.PoseProblem * max(1, len(problems)))()
    R = (L.PoseResult * max(1, len(problems)))()
    keeps = []
    for b, pb in enumerate(problems):
        S[b], R[b], k = _pose_problem(pb)
        keeps.append(k)
    L.check(ctx.lib.ov2_compute_pose_batch(ctx.h, C.byref(_as_pose_params(params)), len(problems), S, R))
    return [_pose_finish(R[b], keeps[b]) for b in range(len(problems))]


def pose_from_model(model):
    """ov2_pose_from_model (host only): [t q(xyzw)] of a P3P model (Rwc row-major, twc), with the arithmetic the chain uses"""
    m = np.ascontiguousarray(model, np.float64).reshape(12)
    out = np.zeros(7, np.float64)
    L.check(L.load().ov2_pose_from_model(_dp(m), _dp(out)))
    return out
