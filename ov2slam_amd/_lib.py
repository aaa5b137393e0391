"""ctypes binding of libov2slam_hip.so (the C ABI declared in include/ov2slam_hip.h).

The product path has no CPU fallback: if the HIP library is missing this module
raises at import of the symbol table, and if no GPU is visible every compute entry
point returns OV2_ENODEVICE which is surfaced as Ov2Error.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("OV2SLAM_HIP_LIB") or os.path.join(_HERE, "libov2slam_hip.so")   # override: A/B builds

OV2_OK = 0
OV2_EINVAL, OV2_EHIP, OV2_ENOMEM, OV2_EUNSUPPORTED, OV2_ENODEVICE = -1, -2, -3, -4, -5
OV2_LK_USE_INITIAL_FLOW = 4
OV2_LK_GET_MIN_EIGENVALS = 8
OV2_MASK_AS_EXECUTED, OV2_MASK_INTENDED = 0, 1
OV2_CAM_PINHOLE, OV2_CAM_FISHEYE = 0, 1
OV2_OPT_SOBEL_DY_ORDER = 1
OV2_SOBEL_DY_OPENCV_ROWFILTER, OV2_SOBEL_DY_EXACT_SUM = 0, 1
# path selection / test forcing (include/ov2slam_hip.h): per context, never through the environment
OV2_OPT_LK_IMPL, OV2_OPT_TRACK_IMPL, OV2_OPT_CLAHE_STRIPS, OV2_OPT_BA_FORCE_LARGE, OV2_OPT_BA_LIN_DIRECT = 2, 3, 4, 5, 6
OV2_OPT_BA_SCHUR_CHUNK, OV2_OPT_BA_XYZ_LIN_WAVES, OV2_OPT_BA_POSE_ONLY_FUSED, OV2_OPT_BA_DETERMINISTIC, OV2_OPT_DEBUG = 7, 8, 9, 10, 11
OV2_OPT_FAST_TIE = 12
OV2_OPT_BA_TRACE = 13
OV2_OPT_LK_ACC = 14
OV2_OPT_DETECT_STRIP = 15
OV2_OPT_LCKF_SCRATCH_KB = 16
OV2_OPT_LK_PERSIST = 17
OV2_OPT_EPIF_CAPACITY = 18
OV2_LK_ACC_INT64, OV2_LK_ACC_FLOAT_UI4 = 0, 1
OV2_FAST_TIE_SCAN_ORDER, OV2_FAST_TIE_LIBSTDCXX = 0, 1
OV2_LK_IMPL_AUTO, OV2_LK_IMPL_ROW, OV2_LK_IMPL_LANE3 = 0, 1, 2
OV2_TRACK_IMPL_WAVE, OV2_TRACK_IMPL_ROW = 0, 1
OV2_BRIEF_BYTES = 32
OV2_MAP_F32, OV2_MAP_FIXED = 0, 1
OV2_RES_LEFT, OV2_RES_RIGHT, OV2_RES_RIGHT_ANCH, OV2_RES_PNP = 0, 1, 2, 3
OV2_TRI_STEREO_TRIED, OV2_TRI_STEREO_OK, OV2_TRI_TEMPORAL_TRIED, OV2_TRI_TEMPORAL_OK, OV2_TRI_NO_MOTION, OV2_TRI_REMOVE_OBS = 1, 2, 4, 8, 16, 32
OV2_MATCH_BEHIND, OV2_MATCH_OUT_OF_FOV, OV2_MATCH_OUT_OF_IMAGE, OV2_MATCH_NO_CANDIDATE, OV2_MATCH_RATIO_REJECTED, OV2_MATCH_BEST = 1, 2, 4, 8, 16, 32
OV2_LOOPMAP_BEHIND, OV2_LOOPMAP_OUT_OF_FOV, OV2_LOOPMAP_OUT_OF_IMAGE = 1, 2, 4
OV2_LOOPMAP_NO_CANDIDATE, OV2_LOOPMAP_RATIO_REJECTED, OV2_LOOPMAP_BEST = 8, 16, 32
# frame versus keyframe (fkf.hip)
OV2_FKF_MAX_POINTS, OV2_FKF_MAX_CELLS = 2048, 65536
OV2_FKF_ALL, OV2_FKF_ONLY_2D, OV2_FKF_ONLY_3D = 0, 1, 2
OV2_FKF_AVG, OV2_FKF_MEDIAN, OV2_FKF_AVG_WIDE = 0, 1, 2
OV2_KF_C0, OV2_KF_C1, OV2_KF_C2, OV2_KF_CX = 1, 2, 4, 8
OV2_KF_RET_FEW_CELLS, OV2_KF_RET_FEW_3D, OV2_KF_RET_MANY_3D, OV2_KF_RET_TIME, OV2_KF_NONFINITE = 16, 32, 64, 128, 256
OV2_KF_FIRST_FRAME, OV2_KF_NO_KEYFRAME = 512, 1024      # ov2_btracker_track_mono
OV2_CKF_DET_SINGLESCALE, OV2_CKF_DET_GRID_FAST, OV2_CKF_DET_GFTT = 0, 1, 2             # ov2_btracker_create_keyframe
OV2_CKF_NOT_REQUESTED, OV2_CKF_CREATED, OV2_CKF_OVERFLOW, OV2_CKF_DUP_LMID = 0, 1, 2, 3
OV2_RES_SET_POINT, OV2_RES_UNSET_POINT, OV2_RES_REMOVE = 0, 1, 2                        # ov2_btracker_update_frame
OV2_SKF_NOT_REQUESTED, OV2_SKF_NOT_KEYFRAME, OV2_SKF_DONE = 0, 1, 2                     # ov2_btracker_stereo_keyframe
OV2_TKF_NOT_REQUESTED, OV2_TKF_NOT_KEYFRAME, OV2_TKF_DONE, OV2_TKF_SRC_OVERFLOW = 0, 1, 2, 3   # ov2_btracker_temporal_keyframe
OV2_TKF_MAX_ROWS = 256
OV2_P3P_LMEDS, OV2_P3P_RANSAC = 0, 1
OV2_P3P_TOO_FEW_POINTS, OV2_P3P_NO_MODEL, OV2_P3P_FEW_INLIERS, OV2_P3P_NOT_ORTHOGONAL = 1, 2, 4, 8
OV2_P3P_MAX_POINTS, OV2_P3P_MAX_ROWS = 2048, 4096
OV2_POSE_TOO_FEW, OV2_POSE_OK, OV2_POSE_PNP_REQ_P3P, OV2_POSE_P3P_RESET, OV2_POSE_PNP_RESET, OV2_POSE_PNP_KEEP = 0, 1, 2, 3, 4, 5
OV2_EPI_TOO_FEW_POINTS, OV2_EPI_NO_MODEL, OV2_EPI_FEW_INLIERS = 1, 2, 4
OV2_EPI_MAX_POINTS, OV2_EPI_MAX_ROWS = 2048, 4096
OV2_EPIF_TOO_FEW_KPS, OV2_EPIF_LOW_PARALLAX, OV2_EPIF_NO_MODEL, OV2_EPIF_DEGENERATE, OV2_EPIF_FILTERED = 0, 1, 2, 3, 4
(OV2_MINIT_RESET, OV2_MINIT_LOW_PARALLAX, OV2_MINIT_TOO_FEW_KPS, OV2_MINIT_TOO_FEW_MATCHES, OV2_MINIT_LOW_ROT_PARALLAX,
 OV2_MINIT_NO_MODEL, OV2_MINIT_READY, OV2_MINIT_NOT_REQUESTED, OV2_MINIT_NO_KEYFRAME) = range(9)
OV2_PG_MAX_POSES, OV2_PG_MAX_EDGES = 16384, 32768
OV2_TERM_NO_CONVERGENCE, OV2_TERM_FUNCTION_TOL, OV2_TERM_PARAMETER_TOL, OV2_TERM_GRADIENT_TOL = 0, 1, 2, 3
OV2_TERM_MIN_RADIUS, OV2_TERM_INVALID_STEPS, OV2_TERM_FAILURE = 4, 5, 6


class Ov2Error(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("ov2slam_hip error %d: %s" % (code, msg))
        self.code = code


class BAProblem(C.Structure):
    _fields_ = [
        ("n_kf", C.c_int), ("poses", C.POINTER(C.c_double)), ("kf_const", C.POINTER(C.c_uint8)),
        ("n_lm", C.c_int), ("invdepth", C.POINTER(C.c_double)), ("lm_anchor_kf", C.POINTER(C.c_int)),
        ("lm_anchor_uv", C.POINTER(C.c_double)),
        ("n_res", C.c_int), ("res_type", C.POINTER(C.c_uint8)), ("res_kf", C.POINTER(C.c_int)),
        ("res_lm", C.POINTER(C.c_int)), ("res_uv", C.POINTER(C.c_double)), ("res_sigma", C.POINTER(C.c_double)),
        ("res_active", C.POINTER(C.c_uint8)), ("res_xyz", C.POINTER(C.c_double)),
        ("calib_l", C.c_double * 4), ("calib_r", C.c_double * 4), ("T_rl", C.c_double * 7),
    ]


class BAOptions(C.Structure):
    _fields_ = [
        ("max_iter", C.c_int), ("function_tolerance", C.c_double), ("gradient_tolerance", C.c_double),
        ("parameter_tolerance", C.c_double), ("huber_delta", C.c_double), ("initial_radius", C.c_double),
        ("max_radius", C.c_double), ("min_radius", C.c_double), ("min_lm_diagonal", C.c_double),
        ("max_lm_diagonal", C.c_double), ("min_relative_decrease", C.c_double), ("jacobi_scaling", C.c_int),
        ("max_consecutive_invalid_steps", C.c_int), ("max_solver_time_s", C.c_double),
    ]


class BAResult(C.Structure):
    _fields_ = [
        ("poses_out", C.POINTER(C.c_double)), ("invdepth_out", C.POINTER(C.c_double)),
        ("chi2_last_eval", C.POINTER(C.c_double)), ("depthpos_last_eval", C.POINTER(C.c_uint8)),
        ("iterations", C.c_int), ("num_successful_steps", C.c_int),
        ("initial_cost", C.c_double), ("final_cost", C.c_double), ("termination", C.c_int),
        ("solve_ms", C.c_double),
    ]


class LocalBAOptions(C.Structure):
    _fields_ = [
        ("robust_mono_th", C.c_double), ("use_robust_cost", C.c_int), ("apply_l2_after_robust", C.c_int),
        ("stop_requested", C.c_int), ("stop_flag", C.POINTER(C.c_int)), ("pass1", BAOptions), ("pass2", BAOptions),
    ]


class LocalBAResult(C.Structure):
    _fields_ = [
        ("poses_out", C.POINTER(C.c_double)), ("invdepth_out", C.POINTER(C.c_double)), ("bad_obs", C.POINTER(C.c_uint8)),
        ("bad_after_pass1", C.POINTER(C.c_uint8)), ("chi2_last_eval", C.POINTER(C.c_double)),
        ("depthpos_last_eval", C.POINTER(C.c_uint8)), ("l2_done", C.c_int), ("pass2_error", C.c_int), ("n_bad_pass1", C.c_int), ("n_bad_total", C.c_int),
        ("iterations", C.c_int * 2), ("num_successful_steps", C.c_int * 2), ("termination", C.c_int * 2), ("initial_cost", C.c_double * 2),
        ("final_cost", C.c_double * 2), ("solve_ms", C.c_double * 2), ("status", C.c_int),
    ]


class BAIter(C.Structure):
    """ov2_ba_iter"""
    _fields_ = [("iteration", C.c_int), ("step_is_valid", C.c_int), ("step_is_successful", C.c_int), ("reserved_", C.c_int),
                ("cost", C.c_double), ("cost_change", C.c_double), ("gradient_max_norm", C.c_double), ("gradient_norm", C.c_double),
                ("step_norm", C.c_double), ("relative_decrease", C.c_double), ("trust_region_radius", C.c_double)]


class SBAProblem(C.Structure):
    _fields_ = [
        ("n_kf", C.c_int), ("poses", C.POINTER(C.c_double)), ("n_pts", C.c_int), ("xyz", C.POINTER(C.c_double)),
        ("n_res", C.c_int), ("res_type", C.POINTER(C.c_uint8)), ("res_kf", C.POINTER(C.c_int)), ("res_pt", C.POINTER(C.c_int)),
        ("res_uv", C.POINTER(C.c_double)), ("res_sigma", C.POINTER(C.c_double)), ("res_active", C.POINTER(C.c_uint8)),
        ("calib_l", C.c_double * 4), ("calib_r", C.c_double * 4), ("T_rl", C.c_double * 7),
    ]


class SBAResult(C.Structure):
    _fields_ = [
        ("xyz_out", C.POINTER(C.c_double)), ("chi2_last_eval", C.POINTER(C.c_double)), ("depthpos_last_eval", C.POINTER(C.c_uint8)),
        ("iterations", C.c_int), ("num_successful_steps", C.c_int), ("initial_cost", C.c_double), ("final_cost", C.c_double),
        ("termination", C.c_int), ("solve_ms", C.c_double),
    ]


class TrackerConfig(C.Structure):
    _fields_ = [
        ("w", C.c_int), ("h", C.c_int), ("win", C.c_int), ("nklt_pyr_lvl", C.c_int), ("prior_pyr_lvl", C.c_int),
        ("max_iter", C.c_int), ("eps", C.c_float), ("err_th", C.c_float), ("fb_dist", C.c_float),
        ("use_clahe", C.c_int), ("clahe_clip", C.c_double), ("tiles_x", C.c_int), ("tiles_y", C.c_int),
        ("n_max", C.c_int), ("use_graph", C.c_int),
    ]


class XYZBAProblem(C.Structure):
    _fields_ = [
        ("n_kf", C.c_int), ("poses", C.POINTER(C.c_double)), ("kf_const", C.POINTER(C.c_uint8)), ("n_pts", C.c_int),
        ("xyz", C.POINTER(C.c_double)), ("n_res", C.c_int), ("res_type", C.POINTER(C.c_uint8)), ("res_kf", C.POINTER(C.c_int)),
        ("res_pt", C.POINTER(C.c_int)), ("res_uv", C.POINTER(C.c_double)), ("res_sigma", C.POINTER(C.c_double)),
        ("res_active", C.POINTER(C.c_uint8)), ("calib_l", C.c_double * 4), ("calib_r", C.c_double * 4), ("T_rl", C.c_double * 7),
    ]


class GfttParams(C.Structure):
    """ov2_gftt_params: FeatureExtractor's nmaxpts_, nmaxdist_, nmindist_, dminquality_, dmaxquality_"""
    _fields_ = [("nmaxpts", C.c_int), ("nmaxdist", C.c_int), ("nmindist", C.c_int),
                ("dminquality", C.c_double), ("dmaxquality", C.c_double)]


class TriParams(C.Structure):
    """ov2_tri_params (Mapper::triangulateStereo / triangulateTemporal)"""
    _fields_ = [("stereo", C.c_int), ("rect", C.c_int), ("fmax_reproj_err", C.c_float), ("K", C.c_double * 4),
                ("iK", C.c_double * 9), ("Kr", C.c_double * 4), ("Tlr", C.c_double * 7), ("Tcic0", C.c_double * 7)]


class TriKeyframe(C.Structure):
    """ov2_tri_keyframe"""
    _fields_ = [("n", C.c_int), ("Twc", C.POINTER(C.c_double)), ("unpx", C.POINTER(C.c_float)), ("bv", C.POINTER(C.c_double)),
                ("is_stereo", C.POINTER(C.c_uint8)), ("runpx", C.POINTER(C.c_float)), ("rbv", C.POINTER(C.c_double)),
                ("src", C.POINTER(C.c_int)), ("src_unpx", C.POINTER(C.c_float)), ("src_bv", C.POINTER(C.c_double)),
                ("n_src", C.c_int), ("src_Twc", C.POINTER(C.c_double)), ("src_Tcw", C.POINTER(C.c_double))]


class TriResult(C.Structure):
    """ov2_tri_result"""
    _fields_ = [("status", C.POINTER(C.c_uint8)), ("wpt", C.POINTER(C.c_double)), ("invdepth", C.POINTER(C.c_double)),
                ("n_stereo", C.c_int), ("n_stereo_good", C.c_int), ("n_candidates", C.c_int), ("n_temporal_good", C.c_int)]


class MatchParams(C.Structure):
    """ov2_match_params (Mapper::matchToMap)"""
    _fields_ = [("model", C.c_int), ("K", C.c_double * 4), ("D", C.POINTER(C.c_double)), ("nD", C.c_int), ("img_w", C.c_double),
                ("img_h", C.c_double), ("ncellsize", C.c_int), ("fmax_proj_pxdist", C.c_float), ("fmax_desc_dist", C.c_float),
                ("desc_bytes", C.c_int)]


class MatchKeyframe(C.Structure):
    """ov2_match_keyframe"""
    _fields_ = [("Tcw", C.POINTER(C.c_double)), ("nb3dkps", C.c_int), ("n_kp", C.c_int), ("kp_px", C.POINTER(C.c_float)),
                ("kp_mp", C.POINTER(C.c_int)), ("cell_start", C.POINTER(C.c_int)), ("cell_kp", C.POINTER(C.c_int)),
                ("n_mp", C.c_int), ("obs_start", C.POINTER(C.c_int)), ("obs_kfid", C.POINTER(C.c_int)),
                ("obs_kf", C.POINTER(C.c_int)), ("obs_px", C.POINTER(C.c_float)), ("desc_start", C.POINTER(C.c_int)),
                ("desc", C.POINTER(C.c_uint8)), ("n_kf", C.c_int), ("kf_Tcw", C.POINTER(C.c_double)), ("n_lm", C.c_int),
                ("lm_mp", C.POINTER(C.c_int)), ("lm_wpt", C.POINTER(C.c_double))]


class MatchResult(C.Structure):
    """ov2_match_result"""
    _fields_ = [("lm_status", C.POINTER(C.c_uint8)), ("lm_kp", C.POINTER(C.c_int)), ("lm_dist", C.POINTER(C.c_float)),
                ("lm_projpx", C.POINTER(C.c_float)), ("kp_lm", C.POINTER(C.c_int)), ("kp_dist", C.POINTER(C.c_float)),
                ("n_matches", C.c_int)]


class KnnParams(C.Structure):
    """ov2_knn_params (LoopCloser::knnMatching)"""
    _fields_ = [("desc_bytes", C.c_int), ("max_dist", C.c_int), ("ratio", C.c_double)]


class KnnItem(C.Structure):
    """ov2_knn_item"""
    _fields_ = [("n_query", C.c_int), ("n_train", C.c_int), ("query", C.POINTER(C.c_uint8)), ("train", C.POINTER(C.c_uint8))]


class KnnResult(C.Structure):
    """ov2_knn_result"""
    _fields_ = [("idx", C.POINTER(C.c_int)), ("dist", C.POINTER(C.c_int)), ("good", C.POINTER(C.c_uint8)),
                ("pair_query", C.POINTER(C.c_int)), ("pair_train", C.POINTER(C.c_int)), ("n_pairs", C.c_int)]


class LoopMapParams(C.Structure):
    """ov2_loopmap_params (LoopCloser::matchToMap)"""
    _fields_ = [("model", C.c_int), ("K", C.c_double * 4), ("D", C.POINTER(C.c_double)), ("nD", C.c_int), ("img_w", C.c_double),
                ("img_h", C.c_double), ("ncellsize", C.c_int), ("fmax_proj_pxdist", C.c_float), ("fmax_desc_dist", C.c_float),
                ("desc_bytes", C.c_int)]


class LoopMapItem(C.Structure):
    """ov2_loopmap_item"""
    _fields_ = [("Tcw", C.POINTER(C.c_double)), ("n_kp", C.c_int), ("kp_px", C.POINTER(C.c_float)), ("kp_mp", C.POINTER(C.c_int)),
                ("kp_matched", C.POINTER(C.c_uint8)), ("cell_start", C.POINTER(C.c_int)), ("cell_kp", C.POINTER(C.c_int)),
                ("n_mp", C.c_int), ("obs_start", C.POINTER(C.c_int)), ("obs_kfid", C.POINTER(C.c_int)),
                ("desc_start", C.POINTER(C.c_int)), ("desc", C.POINTER(C.c_uint8)), ("n_lm", C.c_int),
                ("lm_mp", C.POINTER(C.c_int)), ("lm_wpt", C.POINTER(C.c_double))]


class LoopMapResult(C.Structure):
    """ov2_loopmap_result"""
    _fields_ = [("lm_status", C.POINTER(C.c_uint8)), ("lm_kp", C.POINTER(C.c_int)), ("lm_dist", C.POINTER(C.c_float)),
                ("lm_projpx", C.POINTER(C.c_float)), ("kp_lm", C.POINTER(C.c_int)), ("kp_dist", C.POINTER(C.c_float)),
                ("n_matches", C.c_int)]


class LckfParams(C.Structure):
    """ov2_lckf_params (LoopCloser::run's keyframe preparation)"""
    _fields_ = [("threshold", C.c_int), ("retain", C.c_int), ("excl_radius", C.c_int)]


class LckfResult(C.Structure):
    """ov2_lckf_result"""
    _fields_ = [("n_all", C.c_int), ("cut", C.c_int), ("n_kept", C.c_int), ("n_desc", C.c_int),
                ("all_xy", C.POINTER(C.c_int16)), ("all_resp", C.POINTER(C.c_uint8)), ("all_cap", C.c_int),
                ("kept_xy", C.POINTER(C.c_int16)), ("kept_resp", C.POINTER(C.c_uint8)), ("kept_valid", C.POINTER(C.c_uint8)),
                ("kept_desc", C.POINTER(C.c_uint8)), ("kept_cap", C.c_int)]


class P3PParams(C.Structure):
    """ov2_p3p_params"""
    _fields_ = [("mode", C.c_int), ("max_iterations", C.c_int), ("threshold", C.c_double), ("probability", C.c_double),
                ("boptimize", C.c_int)]


class P3PProblem(C.Structure):
    """ov2_p3p_problem"""
    _fields_ = [("n", C.c_int), ("bv", C.POINTER(C.c_double)), ("X", C.POINTER(C.c_double)), ("n_rows", C.c_int),
                ("samples", C.POINTER(C.c_int))]


class P3PResult(C.Structure):
    """ov2_p3p_result"""
    _fields_ = [("model", C.c_double * 12), ("score", C.c_double), ("best_row", C.c_int), ("iterations", C.c_int),
                ("rows_consumed", C.c_int), ("status", C.c_int), ("n_inliers", C.c_int), ("n_outliers", C.c_int),
                ("outliers", C.POINTER(C.c_int)), ("trace_valid", C.POINTER(C.c_uint8)), ("trace_score", C.POINTER(C.c_double))]


class PnPParams(C.Structure):
    """ov2_pnp_params"""
    _fields_ = [("nmaxiter", C.c_int), ("chi2th", C.c_double), ("use_robust", C.c_int), ("apply_l2_after_robust", C.c_int),
                ("K", C.c_double * 4)]


class PnPProblem(C.Structure):
    """ov2_pnp_problem"""
    _fields_ = [("n", C.c_int), ("unpx", C.POINTER(C.c_double)), ("wpt", C.POINTER(C.c_double)), ("scale", C.POINTER(C.c_int)),
                ("Twc", C.POINTER(C.c_double))]


class PnPPass(C.Structure):
    """ov2_pnp_pass"""
    _fields_ = [("ran", C.c_int), ("iterations", C.c_int), ("num_successful_steps", C.c_int), ("termination", C.c_int),
                ("initial_cost", C.c_double), ("final_cost", C.c_double)]


class PnPResult(C.Structure):
    """ov2_pnp_result"""
    _fields_ = [("success", C.c_int), ("n_outliers", C.c_int), ("Twc", C.c_double * 7), ("outliers", C.POINTER(C.c_int)),
                ("passes", PnPPass * 2)]


class PoseParams(C.Structure):
    """ov2_pose_params"""
    _fields_ = [("pnp", PnPParams), ("p3p", P3PParams), ("mono", C.c_int)]


class PoseProblem(C.Structure):
    """ov2_pose_problem"""
    _fields_ = [("n", C.c_int), ("unpx", C.POINTER(C.c_double)), ("wpt", C.POINTER(C.c_double)), ("scale", C.POINTER(C.c_int)),
                ("Twc", C.POINTER(C.c_double)), ("bv", C.POINTER(C.c_double)), ("do_p3p", C.c_int), ("p3p_req", C.c_int),
                ("n_rows", C.c_int), ("samples", C.POINTER(C.c_int))]


class PoseResult(C.Structure):
    """ov2_pose_result"""
    _fields_ = [("Twc", C.c_double * 7), ("action", C.c_int), ("p3p_req_out", C.c_int), ("n_removed_p3p", C.c_int),
                ("n_outliers_pnp", C.c_int), ("ran_p3p", C.c_int), ("p3p_status", C.c_int), ("p3p_best_row", C.c_int),
                ("p3p_iterations", C.c_int), ("p3p_rows_consumed", C.c_int), ("p3p_score", C.c_double),
                ("removed", C.POINTER(C.c_uint8)), ("passes", PnPPass * 2)]


class FramePoseParams(C.Structure):
    """ov2_frame_pose_params"""
    _fields_ = [("pose", PoseParams), ("dop3p", C.c_int), ("n_rows", C.c_int)]


class FramePoseInput(C.Structure):
    """ov2_frame_pose_input"""
    _fields_ = [("Twc_h", C.POINTER(C.c_double)), ("scale_h", C.POINTER(C.c_int)), ("p3p_req_h", C.POINTER(C.c_uint8)),
                ("seed_h", C.POINTER(C.c_ulonglong))]


class EpipolarParams(C.Structure):
    """ov2_epipolar_params"""
    _fields_ = [("max_iterations", C.c_int), ("threshold", C.c_double), ("probability", C.c_double), ("boptimize", C.c_int)]


class EpipolarProblem(C.Structure):
    """ov2_epipolar_problem"""
    _fields_ = [("n", C.c_int), ("bv1", C.POINTER(C.c_double)), ("bv2", C.POINTER(C.c_double)), ("n_rows", C.c_int),
                ("samples", C.POINTER(C.c_int))]


class EpipolarResult(C.Structure):
    """ov2_epipolar_result"""
    _fields_ = [("model", C.c_double * 12), ("score", C.c_double), ("best_row", C.c_int), ("iterations", C.c_int),
                ("rows_consumed", C.c_int), ("status", C.c_int), ("n_inliers", C.c_int), ("n_outliers", C.c_int),
                ("outliers", C.POINTER(C.c_int)), ("trace_valid", C.POINTER(C.c_uint8)), ("trace_score", C.POINTER(C.c_double)),
                ("trace_model", C.POINTER(C.c_double))]


class PGProblem(C.Structure):
    """ov2_pg_problem"""
    _fields_ = [("n_poses", C.c_int), ("poses", C.POINTER(C.c_double)), ("pose_const", C.POINTER(C.c_uint8)), ("n_edges", C.c_int),
                ("edge_i", C.POINTER(C.c_int)), ("edge_j", C.POINTER(C.c_int)), ("edge_T", C.POINTER(C.c_double)),
                ("edge_sigma", C.POINTER(C.c_double))]


class PGResult(C.Structure):
    """ov2_pg_result"""
    _fields_ = [("poses_out", C.POINTER(C.c_double)), ("iterations", C.c_int), ("num_successful_steps", C.c_int),
                ("initial_cost", C.c_double), ("final_cost", C.c_double), ("termination", C.c_int), ("solve_ms", C.c_double)]


class XYZBAResult(C.Structure):
    _fields_ = [
        ("poses_out", C.POINTER(C.c_double)), ("xyz_out", C.POINTER(C.c_double)), ("chi2_last_eval", C.POINTER(C.c_double)),
        ("depthpos_last_eval", C.POINTER(C.c_uint8)), ("iterations", C.c_int), ("num_successful_steps", C.c_int),
        ("initial_cost", C.c_double), ("final_cost", C.c_double), ("termination", C.c_int), ("solve_ms", C.c_double),
    ]


class FkfParams(C.Structure):
    """ov2_fkf_params"""
    _fields_ = [("K", C.c_double * 4), ("ncellsize", C.c_int), ("nbwcells", C.c_int), ("nbhcells", C.c_int), ("nbmaxkps", C.c_int),
                ("finit_parallax", C.c_float), ("stereo", C.c_int)]


class FkfItem(C.Structure):
    """ov2_fkf_item"""
    _fields_ = [("n_cur", C.c_int), ("cur_lmid", C.POINTER(C.c_int)), ("cur_px", C.POINTER(C.c_float)),
                ("cur_unpx", C.POINTER(C.c_float)), ("cur_bv", C.POINTER(C.c_double)), ("cur_is3d", C.POINTER(C.c_uint8)),
                ("cur_Twc", C.POINTER(C.c_double)), ("n_kf", C.c_int), ("kf_lmid", C.POINTER(C.c_int)),
                ("kf_unpx", C.POINTER(C.c_float)), ("kf_Tcw", C.POINTER(C.c_double)), ("cur_id", C.c_int), ("kf_id", C.c_int),
                ("cur_time", C.c_double), ("kf_time", C.c_double), ("kf_nb3dkps", C.c_int), ("localba_is_on", C.c_int),
                ("noccupcells", C.c_int), ("nb3dkps", C.c_int)]


class ParallaxResult(C.Structure):
    """ov2_parallax_result"""
    _fields_ = [("parallax", C.c_float), ("n", C.c_int), ("n_distinct", C.c_int), ("n_nonfinite", C.c_int)]


class KfDecisionResult(C.Structure):
    """ov2_kf_decision_result"""
    _fields_ = [("parallax", C.c_float), ("n", C.c_int), ("n_distinct", C.c_int), ("n_nonfinite", C.c_int),
                ("noccupcells", C.c_int), ("nb3dkps", C.c_int), ("n_out_of_grid", C.c_int), ("decision", C.c_int),
                ("reason", C.c_int)]


class Sampson2dResult(C.Structure):
    """ov2_sampson2d_result"""
    _fields_ = [("err", C.POINTER(C.c_float)), ("bad", C.POINTER(C.c_uint8)), ("n_bad", C.c_int)]


class EpifilterParams(C.Structure):
    """ov2_epifilter_params"""
    _fields_ = [("fkf", FkfParams), ("epi", EpipolarParams), ("fransac_err", C.c_float), ("mono", C.c_int), ("n_rows", C.c_int)]


class EpifilterItem(C.Structure):
    """ov2_epifilter_item"""
    _fields_ = [("fkf", FkfItem), ("kf_bv", C.POINTER(C.c_double)), ("kf_Twc", C.POINTER(C.c_double)), ("nbkfs", C.c_int),
                ("seed", C.c_ulonglong)]


class EpifilterResult(C.Structure):
    """ov2_epifilter_result"""
    _fields_ = [("action", C.c_int), ("m", C.c_int), ("epifrom3dkps", C.c_int), ("do_optimize", C.c_int), ("nb3dkps", C.c_int),
                ("parallax", C.c_float), ("status", C.c_int), ("best_row", C.c_int), ("iterations", C.c_int),
                ("rows_consumed", C.c_int), ("score", C.c_double), ("n_inliers", C.c_int), ("n_outliers", C.c_int),
                ("model", C.c_double * 12), ("F", C.c_double * 9), ("n_removed_ransac", C.c_int), ("n_removed_sampson", C.c_int),
                ("removed", C.POINTER(C.c_uint8)), ("pair_cur", C.POINTER(C.c_int)), ("err", C.POINTER(C.c_float)),
                ("pose_from_model", C.c_int), ("Twc_model", C.c_double * 7), ("trace_samples", C.POINTER(C.c_int))]


class MonoInitParams(C.Structure):
    """ov2_mono_init_params"""
    _fields_ = [("fkf", FkfParams), ("epi", EpipolarParams), ("n_rows", C.c_int), ("min_2d_kps", C.c_int)]


class MonoInitItem(C.Structure):
    """ov2_mono_init_item"""
    _fields_ = [("fkf", FkfItem), ("kf_bv", C.POINTER(C.c_double)), ("seed", C.c_ulonglong)]


class MonoInitResult(C.Structure):
    """ov2_mono_init_result"""
    _fields_ = [("action", C.c_int), ("nb2dkps", C.c_int), ("p0", C.c_float), ("p0_n", C.c_int), ("p0_n_distinct", C.c_int),
                ("p0_n_nonfinite", C.c_int), ("m", C.c_int), ("p1", C.c_float), ("status", C.c_int), ("best_row", C.c_int),
                ("iterations", C.c_int), ("rows_consumed", C.c_int), ("score", C.c_double), ("n_inliers", C.c_int),
                ("n_outliers", C.c_int), ("model", C.c_double * 12), ("n_removed", C.c_int), ("pose_refined", C.c_int),
                ("Twc_init", C.c_double * 7), ("removed", C.POINTER(C.c_uint8)), ("pair_cur", C.POINTER(C.c_int)),
                ("trace_samples", C.POINTER(C.c_int))]


class FrameEpiPoseParams(C.Structure):
    """ov2_frame_epi_pose_params"""
    _fields_ = [("pose", FramePoseParams), ("epi", EpifilterParams)]


class FrameEpiPoseInput(C.Structure):
    """ov2_frame_epi_pose_input"""
    _fields_ = [("pose", FramePoseInput), ("lmid_h", C.POINTER(C.c_int)), ("nbkfs_h", C.POINTER(C.c_int)),
                ("epi_seed_h", C.POINTER(C.c_ulonglong))]


class MotionState(C.Structure):
    """ov2_motion_state"""
    _fields_ = [("prev_time", C.c_double), ("prevTwc", C.c_double * 7), ("log_relT", C.c_double * 6)]


class TrackMonoParams(C.Structure):
    """ov2_track_mono_params"""
    _fields_ = [("step", FrameEpiPoseParams), ("doepipolar", C.c_int)]


class TrackMonoInput(C.Structure):
    """ov2_track_mono_input"""
    _fields_ = [("step", FrameEpiPoseInput), ("time_h", C.POINTER(C.c_double)), ("frame_id_h", C.POINTER(C.c_int)),
                ("localba_is_on_h", C.POINTER(C.c_uint8))]


class TrackMonoResult(C.Structure):
    """ov2_track_mono_result"""
    _fields_ = [("Twc_pred", C.c_double * 7), ("resynced", C.c_int), ("state", MotionState), ("kf", KfDecisionResult)]


class CreateKeyframeParams(C.Structure):
    """ov2_create_keyframe_params"""
    _fields_ = [("ncellsize", C.c_int), ("nbwcells", C.c_int), ("nbhcells", C.c_int), ("nbmaxkps", C.c_int), ("detector", C.c_int),
                ("det_cell", C.c_int), ("roi", C.c_int * 4), ("mask_mode", C.c_int), ("do_subpix", C.c_int), ("use_brief", C.c_int)]


class CreateKeyframeInput(C.Structure):
    """ov2_create_keyframe_input"""
    _fields_ = [("px_h", C.POINTER(C.c_float)), ("lmid_h", C.POINTER(C.c_int)), ("is3d_h", C.POINTER(C.c_uint8)), ("n_h", C.POINTER(C.c_int)),
                ("make_kf_h", C.POINTER(C.c_uint8)), ("nlmid_h", C.POINTER(C.c_int)), ("nkfid_h", C.POINTER(C.c_int)),
                ("time_h", C.POINTER(C.c_double)), ("Twc_h", C.POINTER(C.c_double)), ("quality_inout", C.POINTER(C.c_double)),
                ("fast_th_inout", C.POINTER(C.c_int))]


class CreateKeyframeResult(C.Structure):
    """ov2_create_keyframe_result"""
    _fields_ = [("action", C.c_int), ("n_prev", C.c_int), ("noccupcells", C.c_int), ("nb2detect", C.c_int), ("n_new", C.c_int),
                ("n_kf", C.c_int), ("nb3dkps", C.c_int), ("pad", C.c_int)]


class ResidentOp(C.Structure):
    """ov2_resident_op"""
    _fields_ = [("lmid", C.c_int), ("op", C.c_int), ("xyz", C.c_double * 3)]


class ResidentUpdateResult(C.Structure):
    """ov2_resident_update_result"""
    _fields_ = [("n_before", C.c_int), ("n_after", C.c_int), ("n_set", C.c_int), ("n_unset", C.c_int), ("n_removed", C.c_int),
                ("n_missing", C.c_int)]


class ResidentStepResult(C.Structure):
    """ov2_resident_step_result"""
    _fields_ = [("n_before", C.c_int), ("n_after", C.c_int)]


class StereoKeyframeParams(C.Structure):
    """ov2_stereo_keyframe_params"""
    _fields_ = [("nklt_win_size", C.c_int), ("nklt_pyr_lvl", C.c_int), ("max_iter", C.c_int), ("eps", C.c_float), ("nklt_err", C.c_float),
                ("fmax_fbklt_dist", C.c_float), ("rect", C.c_int), ("Frl", C.c_double * 9), ("model", C.c_int), ("K", C.c_double * 4),
                ("D", C.POINTER(C.c_double)), ("nD", C.c_int), ("iK", C.c_double * 9), ("img_w", C.c_double), ("img_h", C.c_double),
                ("Tcic0", C.c_double * 7), ("ncellsize", C.c_int), ("tri", TriParams)]


class StereoKeyframeResult(C.Structure):
    """ov2_stereo_keyframe_result"""
    _fields_ = [("action", C.c_int), ("n", C.c_int), ("n_prior3d", C.c_int), ("n_prior_nb", C.c_int), ("n_stereo_kps", C.c_int),
                ("n_stereo", C.c_int), ("n_stereo_good", C.c_int), ("nb3dkps", C.c_int)]


class TemporalKeyframeParams(C.Structure):
    """ov2_temporal_keyframe_params"""
    _fields_ = [("tri", TriParams), ("n_src_max", C.c_int)]


class TemporalKeyframeResult(C.Structure):
    """ov2_temporal_keyframe_result"""
    _fields_ = [("action", C.c_int), ("n", C.c_int), ("n_candidates", C.c_int), ("n_temporal_good", C.c_int), ("n_remove_obs", C.c_int),
                ("n_no_motion", C.c_int), ("nb3dkps", C.c_int), ("n_rows", C.c_int)]


class KltPriorsParams(C.Structure):
    """ov2_klt_priors_params"""
    _fields_ = [("model", C.c_int), ("K", C.c_double * 4), ("D", C.POINTER(C.c_double)), ("nD", C.c_int), ("img_w", C.c_double),
                ("img_h", C.c_double), ("klt_use_prior", C.c_int)]


class KltPriorsItem(C.Structure):
    """ov2_klt_priors_item"""
    _fields_ = [("Tcw", C.POINTER(C.c_double)), ("n", C.c_int), ("px", C.POINTER(C.c_float)), ("is3d", C.POINTER(C.c_uint8)),
                ("wpt", C.POINTER(C.c_double))]


class KltPriorsResult(C.Structure):
    """ov2_klt_priors_result"""
    _fields_ = [("prior", C.POINTER(C.c_float)), ("has_prior", C.POINTER(C.c_uint8)), ("n_prior", C.c_int)]


class StereoPriorsParams(C.Structure):
    """ov2_stereo_priors_params"""
    _fields_ = [("model", C.c_int), ("K", C.c_double * 4), ("D", C.POINTER(C.c_double)), ("nD", C.c_int), ("img_w", C.c_double),
                ("img_h", C.c_double), ("Tcic0", C.c_double * 7), ("ncellsize", C.c_int), ("rect", C.c_int)]


class StereoPriorsItem(C.Structure):
    """ov2_stereo_priors_item"""
    _fields_ = [("Tcw", C.POINTER(C.c_double)), ("n", C.c_int), ("px", C.POINTER(C.c_float)), ("unpx", C.POINTER(C.c_float)),
                ("bv", C.POINTER(C.c_double)), ("wpt", C.POINTER(C.c_double)), ("state", C.POINTER(C.c_uint8)),
                ("cell_start", C.POINTER(C.c_int)), ("cell_kp", C.POINTER(C.c_int))]


class StereoPriorsResult(C.Structure):
    """ov2_stereo_priors_result"""
    _fields_ = [("prior", C.POINTER(C.c_float)), ("has_prior", C.POINTER(C.c_uint8)), ("skip", C.POINTER(C.c_uint8)),
                ("n_prior3d", C.c_int), ("n_prior_nb", C.c_int), ("n_skip", C.c_int)]


_vp, _i, _f, _d = C.c_void_p, C.c_int, C.c_float, C.c_double
_pp = C.POINTER(C.c_void_p)

# name -> (restype, argtypes).  Must list every symbol include/ov2slam_hip.h declares
# (tests/test_abi.py cross-checks this table against the header).
SIGNATURES = {
    "ov2_version": (_i, []),
    "ov2_last_error": (C.c_char_p, []),
    "ov2_ctx_create": (_i, [_i, _pp]),
    "ov2_ctx_create_with_priority": (_i, [_i, _i, _pp]),
    "ov2_ctx_create_on_stream": (_i, [_i, _vp, _pp]),
    "ov2_ctx_destroy": (None, [_vp]),
    "ov2_ctx_sync": (_i, [_vp]),
    "ov2_ctx_stream": (_vp, [_vp]),
    "ov2_ctx_set_option": (_i, [_vp, _i, _i]),
    "ov2_ctx_get_option": (_i, [_vp, _i, C.POINTER(C.c_int)]),
    "ov2_pyr_create": (_i, [_vp, _i, _i, _i, _i, _i, _pp]),
    "ov2_pyr_destroy": (None, [_vp]),
    "ov2_pyr_levels": (_i, [_vp]),
    "ov2_pyr_level_size": (_i, [_vp, _i, C.POINTER(_i), C.POINTER(_i)]),
    "ov2_pyr_batch": (_i, [_vp]),
    "ov2_pyr_item_view": (_i, [_vp, _i, _pp]),
    "ov2_pyr_build_h": (_i, [_vp, _vp, _vp, _i, C.c_size_t]),
    "ov2_pyr_build_d": (_i, [_vp, _vp, _vp, _i, C.c_size_t]),
    "ov2_pyr_download": (_i, [_vp, _vp, _i, _i, _vp, _vp]),
    "ov2_pyr_download_padded": (_i, [_vp, _vp, _i, _i, _vp, _vp]),
    "ov2_pyr_algorithmic_bytes": (C.c_size_t, [_vp]),
    "ov2_clahe_h": (_i, [_vp, _vp, _i, _i, _i, _d, _i, _i, _vp, _i]),
    "ov2_clahe_d": (_i, [_vp, _vp, _i, _i, _i, C.c_size_t, _i, _d, _i, _i, _vp, _i, C.c_size_t]),
    "ov2_compute_keypoints": (_i, [_vp, _i, _vp, _vp, _i, _vp, _vp, _i, _vp, _vp]),
    "ov2_compute_keypoints_d": (_i, [_vp, _i, _vp, _vp, _i, _vp, _vp, _i, _vp, _vp]),
    "ov2_line_min_sad": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp, _i, _vp, _vp]),
    "ov2_stereo_epipolar_check": (_i, [_vp, _i, _vp, _i, _vp, _vp, _i, _vp, _vp, _i, _vp, _vp, _vp]),
    "ov2_stereo_match": (_i, [_vp, _vp, _vp, _i, _i, _i, _f, _f, _f, _i, _vp, _i, _vp, _vp, _i, _vp, _vp, _vp, _vp, _i, _vp, _vp]),
    "ov2_pyr_build_clahe_d": (_i, [_vp, _vp, _vp, _i, C.c_size_t, _d, _i, _i]),
    "ov2_pyr_build_clahe_h": (_i, [_vp, _vp, _vp, _i, _d, _i, _i]),
    "ov2_pyr_build_clahe_hb": (_i, [_vp, _vp, _i, _vp, _i, _d, _i, _i]),
    "ov2_rectmap_create": (_i, [_vp, _i, _i, _i, _vp, _vp, _pp]),
    "ov2_rectmap_destroy": (None, [_vp]),
    "ov2_rectify_h": (_i, [_vp, _vp, _vp, _i, _vp, _i]),
    "ov2_rectify_d": (_i, [_vp, _vp, _vp, C.c_size_t, C.c_size_t, _i, _vp, C.c_size_t, C.c_size_t]),
    "ov2_pyr_build_rect_h": (_i, [_vp, _vp, _vp, _i, _vp, _i, _i, _d, _i, _i]),
    "ov2_stereo_match_batch": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _f, _f, _f, _i, _vp, _i, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "ov2_tracker_create": (_i, [_vp, C.POINTER(TrackerConfig), _pp]),
    "ov2_tracker_destroy": (None, [_vp]),
    "ov2_tracker_image_buffer": (_vp, [_vp, C.POINTER(_i)]),
    "ov2_tracker_preprocess": (_i, [_vp, _vp, _i]),
    "ov2_tracker_klt": (_i, [_vp, _vp, _vp, _vp, _i, _i, _vp, _vp, C.POINTER(_i)]),
    "ov2_tracker_track_frame": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _i, _i, _vp, _vp, C.POINTER(_i)]),
    "ov2_tracker_set_calibration": (_i, [_vp, _i, _vp, _vp, _i, _vp]),
    "ov2_tracker_last_keypoints": (_i, [_vp, _i, _vp, _vp]),
    "ov2_tracker_set_rectification": (_i, [_vp, _vp]),
    "ov2_tracker_cur_pyr": (_vp, [_vp]),
    "ov2_tracker_prev_pyr": (_vp, [_vp]),
    "ov2_tracker_frames": (_i, [_vp]),
    "ov2_tracker_uses_graph": (_i, [_vp]),
    "ov2_btracker_create": (_i, [_vp, C.POINTER(TrackerConfig), _i, _pp]),
    "ov2_btracker_destroy": (None, [_vp]),
    "ov2_btracker_batch": (_i, [_vp]),
    "ov2_btracker_frames": (_i, [_vp]),
    "ov2_btracker_image_buffer": (_vp, [_vp, _i, _i, C.POINTER(_i)]),
    "ov2_btracker_upload": (_i, [_vp, _i, _i]),
    "ov2_btracker_prepare": (_i, [_vp, _i, _i]),
    "ov2_btracker_set_calibration": (_i, [_vp, _i, _vp, _vp, _i, _vp]),
    "ov2_btracker_set_rectification": (_i, [_vp, _vp]),
    "ov2_btracker_track_frame": (_i, [_vp, _i, _vp, _i, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp]),
    "ov2_btracker_track_frame_begin": (_i, [_vp, _i, _vp, _i, _vp, _vp, _vp, _vp, _i]),
    "ov2_btracker_track_frame_end": (_i, [_vp, _vp, _vp, _vp]),
    "ov2_btracker_last_keypoints": (_i, [_vp, _i, _i, _vp, _vp]),
    "ov2_btracker_detect_singlescale": (_i, [_vp, _i, _i, _vp, _vp, C.POINTER(_i), _vp, _i, _vp, _i, _vp]),
    "ov2_btracker_detect_grid_fast": (_i, [_vp, _i, _i, _vp, _vp, _vp, _i, _i, _vp, _i, _vp]),
    "ov2_btracker_pyramid_sets": (_i, [_vp]),
    "ov2_btracker_cur_pyr": (_vp, [_vp]),
    "ov2_btracker_prev_pyr": (_vp, [_vp]),
    "ov2_btracker_cur_item": (_vp, [_vp, _i]),
    "ov2_btracker_prev_item": (_vp, [_vp, _i]),
    "ov2_lk_track": (_i, [_vp, _vp, _vp, _i, _i, _i, _f, _i, _vp, _vp, _i, _vp, _vp, _vp]),
    "ov2_fb_klt": (_i, [_vp, _vp, _vp, _i, _i, _i, _f, _f, _f, _vp, _vp, _i, _vp, _vp]),
    "ov2_fb_klt_d": (_i, [_vp, _vp, _vp, _i, _i, _i, _f, _f, _f, _vp, _vp, _i, _vp, _vp, _vp]),
    "ov2_detect_grid_fast": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _i, C.POINTER(_i), _i, _i, _vp, C.POINTER(_i)]),
    "ov2_detect_singlescale": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _i, C.POINTER(_i), C.POINTER(_d), _i, _vp, C.POINTER(_i)]),
    "ov2_detect_grid_fast_d": (_i, [_vp, _vp, _i, _i, _vp, _i, C.POINTER(_i), _i, _i, _vp, C.POINTER(_i)]),
    "ov2_detect_singlescale_d": (_i, [_vp, _vp, _i, _i, _vp, _i, C.POINTER(_i), C.POINTER(_d), _i, _vp, C.POINTER(_i)]),
    "ov2_detect_singlescale_batch_d": (_i, [_vp, _vp, _i, _vp, _i, _vp, C.POINTER(_i), _vp, _i, _vp, _i, _vp]),
    "ov2_detect_grid_fast_batch_d": (_i, [_vp, _vp, _i, _vp, _i, _vp, _vp, _i, _i, _vp, _i, _vp]),
    "ov2_corner_subpix": (_i, [_vp, _vp, _i, _i, _i, _vp, _i, _i, _i, _d]),
    "ov2_gftt_params_init": (_i, [_i, _i, _d, _vp]),
    "ov2_detect_gftt": (_i, [_vp, _vp, _i, _i, _i, _vp, _i, _vp, _vp, _i, _i, _i, _vp, _i, C.POINTER(_i)]),
    "ov2_detect_gftt_d": (_i, [_vp, _vp, _i, _vp, _i, _vp, _vp, _i, _i, _i, _vp, _i, C.POINTER(_i)]),
    "ov2_detect_gftt_batch_d": (_i, [_vp, _vp, _vp, _i, _vp, _vp, _i, _vp, _vp, _i, _vp, _i, _vp]),
    "ov2_btracker_detect_gftt": (_i, [_vp, _i, _vp, _i, _vp, _vp, _vp, _vp, _i, _vp, _i, _vp]),
    "ov2_set_mask": (_i, [_vp, _i, _i, _i, _vp, _i, _i]),
    "ov2_brief_set_pattern": (_i, [_vp, _vp]),
    "ov2_brief_get_pattern": (_i, [_vp, _vp]),
    "ov2_describe_brief": (_i, [_vp, _vp, _i, _i, _i, _vp, _i, _vp, _vp]),
    "ov2_describe_brief_batch_d": (_i, [_vp, _vp, _i, _i, _i, C.c_size_t, _i, _vp, _i, _vp, _vp, _vp]),
    "ov2_tracker_describe_brief": (_i, [_vp, _vp, _i, _vp, _vp]),
    "ov2_btracker_describe_brief": (_i, [_vp, _i, _vp, _vp, _i, _vp, _vp]),
    "ov2_ba_default_options": (None, [C.POINTER(BAOptions)]),
    "ov2_structure_ba": (_i, [_vp, C.POINTER(SBAProblem), C.POINTER(BAOptions), C.POINTER(SBAResult)]),
    "ov2_xyz_ba_solve": (_i, [_vp, C.POINTER(XYZBAProblem), C.POINTER(BAOptions), C.POINTER(XYZBAResult)]),
    "ov2_ba_solve": (_i, [_vp, C.POINTER(BAProblem), C.POINTER(BAOptions), C.POINTER(BAResult)]),
    "ov2_ba_get_trace": (_i, [_vp, C.POINTER(BAIter), _i, C.POINTER(_i)]),
    "ov2_ba_create": (_i, [_vp, C.POINTER(BAProblem), _pp]),
    "ov2_ba_solve_resident": (_i, [_vp, _vp, C.POINTER(BAOptions), C.POINTER(BAResult)]),
    "ov2_ba_destroy": (None, [_vp]),
    "ov2_local_ba_default_options": (None, [C.POINTER(LocalBAOptions)]),
    "ov2_local_ba": (_i, [_vp, C.POINTER(BAProblem), C.POINTER(LocalBAOptions), C.POINTER(LocalBAResult)]),
    "ov2_local_ba_batch": (_i, [_vp, _i, C.POINTER(BAProblem), C.POINTER(LocalBAOptions), C.POINTER(LocalBAResult), C.POINTER(_i)]),
    "ov2_triangulate_keyframe": (_i, [_vp, C.POINTER(TriParams), C.POINTER(TriKeyframe), C.POINTER(TriResult)]),
    "ov2_triangulate_keyframe_batch": (_i, [_vp, C.POINTER(TriParams), _i, C.POINTER(TriKeyframe), C.POINTER(TriResult)]),
    "ov2_match_to_map": (_i, [_vp, C.POINTER(MatchParams), C.POINTER(MatchKeyframe), C.POINTER(MatchResult)]),
    "ov2_match_to_map_batch": (_i, [_vp, C.POINTER(MatchParams), _i, C.POINTER(MatchKeyframe), C.POINTER(MatchResult)]),
    "ov2_knn_match": (_i, [_vp, C.POINTER(KnnParams), C.POINTER(KnnItem), C.POINTER(KnnResult)]),
    "ov2_knn_match_batch": (_i, [_vp, C.POINTER(KnnParams), _i, C.POINTER(KnnItem), C.POINTER(KnnResult)]),
    "ov2_loop_match_to_map": (_i, [_vp, C.POINTER(LoopMapParams), C.POINTER(LoopMapItem), C.POINTER(LoopMapResult)]),
    "ov2_loop_match_to_map_batch": (_i, [_vp, C.POINTER(LoopMapParams), _i, C.POINTER(LoopMapItem), C.POINTER(LoopMapResult)]),
    "ov2_lckf_params_init": (_i, [C.POINTER(LckfParams)]),
    "ov2_lckf_prepare": (_i, [_vp, _vp, _i, _i, _i, C.POINTER(LckfParams), _vp, _i, C.POINTER(LckfResult)]),
    "ov2_tracker_lckf_prepare": (_i, [_vp, C.POINTER(LckfParams), _vp, _i, C.POINTER(LckfResult)]),
    "ov2_lckf_prepare_batch_d": (_i, [_vp, C.POINTER(LckfParams), _vp, _i, _i, _i, C.c_size_t, _i, _vp, _i, _vp,
                                      _vp, _vp, _i, _vp, _vp, _vp, _vp, _i, _vp]),
    "ov2_btracker_lckf_prepare": (_i, [_vp, _i, C.POINTER(LckfParams), _vp, _vp, _i, C.POINTER(LckfResult)]),
    "ov2_p3p_ransac": (_i, [_vp, C.POINTER(P3PParams), C.POINTER(P3PProblem), C.POINTER(P3PResult)]),
    "ov2_p3p_ransac_batch": (_i, [_vp, C.POINTER(P3PParams), _i, C.POINTER(P3PProblem), C.POINTER(P3PResult)]),
    "ov2_p3p_draw_samples": (_i, [C.c_ulonglong, _i, _i, C.POINTER(_i)]),
    "ov2_ceres_pnp": (_i, [_vp, C.POINTER(PnPParams), C.POINTER(PnPProblem), C.POINTER(PnPResult)]),
    "ov2_ceres_pnp_batch": (_i, [_vp, C.POINTER(PnPParams), _i, C.POINTER(PnPProblem), C.POINTER(PnPResult)]),
    "ov2_compute_pose": (_i, [_vp, C.POINTER(PoseParams), C.POINTER(PoseProblem), C.POINTER(PoseResult)]),
    "ov2_compute_pose_batch": (_i, [_vp, C.POINTER(PoseParams), _i, C.POINTER(PoseProblem), C.POINTER(PoseResult)]),
    "ov2_pose_from_model": (_i, [C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "ov2_epipolar_ransac": (_i, [_vp, C.POINTER(EpipolarParams), C.POINTER(EpipolarProblem), C.POINTER(EpipolarResult)]),
    "ov2_epipolar_ransac_batch": (_i, [_vp, C.POINTER(EpipolarParams), _i, C.POINTER(EpipolarProblem), C.POINTER(EpipolarResult)]),
    "ov2_epipolar_draw_samples": (_i, [C.c_ulonglong, _i, _i, C.POINTER(_i)]),
    "ov2_pose_graph_solve": (_i, [_vp, C.POINTER(PGProblem), C.POINTER(BAOptions), C.POINTER(PGResult)]),
    "ov2_pose_graph_solve_batch": (_i, [_vp, _i, C.POINTER(PGProblem), C.POINTER(BAOptions), C.POINTER(PGResult)]),
    "ov2_pose_graph_apply": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _i, _vp, _vp, _i, _vp, _vp, _vp]),
    "ov2_parallax": (_i, [_vp, C.POINTER(FkfParams), C.POINTER(FkfItem), _i, _i, _i, C.POINTER(ParallaxResult)]),
    "ov2_parallax_batch": (_i, [_vp, C.POINTER(FkfParams), _i, C.POINTER(FkfItem), _i, _i, _i, C.POINTER(ParallaxResult)]),
    "ov2_kf_decision": (_i, [_vp, C.POINTER(FkfParams), C.POINTER(FkfItem), C.POINTER(KfDecisionResult)]),
    "ov2_kf_decision_batch": (_i, [_vp, C.POINTER(FkfParams), _i, C.POINTER(FkfItem), C.POINTER(KfDecisionResult)]),
    "ov2_sampson_filter_2d": (_i, [_vp, C.POINTER(FkfItem), C.POINTER(_d), _f, C.POINTER(Sampson2dResult)]),
    "ov2_sampson_filter_2d_batch": (_i, [_vp, _i, C.POINTER(FkfItem), C.POINTER(_d), _f, C.POINTER(Sampson2dResult)]),
    "ov2_epipolar_filter": (_i, [_vp, C.POINTER(EpifilterParams), C.POINTER(EpifilterItem), C.POINTER(EpifilterResult)]),
    "ov2_epipolar_filter_batch": (_i, [_vp, C.POINTER(EpifilterParams), _i, C.POINTER(EpifilterItem), C.POINTER(EpifilterResult)]),
    "ov2_mono_init": (_i, [_vp, C.POINTER(MonoInitParams), C.POINTER(MonoInitItem), C.POINTER(MonoInitResult)]),
    "ov2_mono_init_batch": (_i, [_vp, C.POINTER(MonoInitParams), _i, C.POINTER(MonoInitItem), C.POINTER(MonoInitResult)]),
    "ov2_btracker_mono_init_begin": (_i, [_vp, _i, C.POINTER(MonoInitParams), _vp, _vp]),
    "ov2_btracker_mono_init_end": (_i, [_vp, C.POINTER(MonoInitResult), _vp]),
    "ov2_btracker_mono_init": (_i, [_vp, _i, C.POINTER(MonoInitParams), _vp, _vp, C.POINTER(MonoInitResult), _vp]),
    "ov2_klt_priors": (_i, [_vp, C.POINTER(KltPriorsParams), C.POINTER(KltPriorsItem), C.POINTER(KltPriorsResult)]),
    "ov2_klt_priors_batch": (_i, [_vp, C.POINTER(KltPriorsParams), _i, C.POINTER(KltPriorsItem), C.POINTER(KltPriorsResult)]),
    "ov2_stereo_priors": (_i, [_vp, C.POINTER(StereoPriorsParams), C.POINTER(StereoPriorsItem), C.POINTER(StereoPriorsResult)]),
    "ov2_stereo_priors_batch": (_i, [_vp, C.POINTER(StereoPriorsParams), _i, C.POINTER(StereoPriorsItem), C.POINTER(StereoPriorsResult)]),
    "ov2_btracker_track_frame_map_begin": (_i, [_vp, _i, _vp, _i, _vp, _vp, _vp, _vp, _vp, _i]),
    "ov2_btracker_track_frame_map": (_i, [_vp, _i, _vp, _i, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp]),
    "ov2_btracker_last_priors": (_i, [_vp, _i, _i, _vp, _vp]),
    "ov2_btracker_track_frame_pose_begin": (_i, [_vp, _i, _vp, _i, _vp, _vp, _vp, _vp, _vp, _i, C.POINTER(FramePoseParams),
                                                 C.POINTER(FramePoseInput)]),
    "ov2_btracker_track_frame_pose_end": (_i, [_vp, _vp, _vp, _vp, C.POINTER(PoseResult)]),
    "ov2_btracker_track_frame_pose": (_i, [_vp, _i, _vp, _i, _vp, _vp, _vp, _vp, _vp, _i, C.POINTER(FramePoseParams),
                                           C.POINTER(FramePoseInput), _vp, _vp, _vp, C.POINTER(PoseResult)]),
    "ov2_btracker_last_pose_inputs": (_i, [_vp, _i, C.POINTER(_i), C.POINTER(_i), C.POINTER(_i), C.POINTER(_i)]),
    "ov2_btracker_set_keyframe": (_i, [_vp, _i, _i, _vp, _vp, _vp, _vp]),
    "ov2_btracker_track_frame_epi_pose_begin": (_i, [_vp, _i, _vp, _i, _vp, _vp, _vp, _vp, _vp, _i, C.POINTER(FrameEpiPoseParams),
                                                     C.POINTER(FrameEpiPoseInput)]),
    "ov2_btracker_track_frame_epi_pose_end": (_i, [_vp, _vp, _vp, _vp, C.POINTER(EpifilterResult), C.POINTER(PoseResult)]),
    "ov2_btracker_track_frame_epi_pose": (_i, [_vp, _i, _vp, _i, _vp, _vp, _vp, _vp, _vp, _i, C.POINTER(FrameEpiPoseParams),
                                               C.POINTER(FrameEpiPoseInput), _vp, _vp, _vp, C.POINTER(EpifilterResult),
                                               C.POINTER(PoseResult)]),
    "ov2_btracker_last_epi_inputs": (_i, [_vp, _i, C.POINTER(_i), C.POINTER(_i), C.POINTER(_i), C.POINTER(_i), C.POINTER(_i)]),
    "ov2_se3_inverse": (_i, [_vp, _vp]),
    "ov2_motion_apply": (_i, [_vp, C.POINTER(MotionState), _vp, _d, C.POINTER(MotionState), _vp, _vp, _vp]),
    "ov2_motion_apply_batch": (_i, [_vp, _i, C.POINTER(MotionState), _vp, _vp, C.POINTER(MotionState), _vp, _vp, _vp]),
    "ov2_motion_update": (_i, [_vp, C.POINTER(MotionState), _vp, _d, C.POINTER(MotionState)]),
    "ov2_motion_update_batch": (_i, [_vp, _i, C.POINTER(MotionState), _vp, _vp, C.POINTER(MotionState)]),
    "ov2_btracker_set_pose": (_i, [_vp, _i, _vp]),
    "ov2_btracker_get_pose": (_i, [_vp, _i, _vp]),
    "ov2_btracker_reset_motion": (_i, [_vp, _i]),
    "ov2_btracker_get_motion": (_i, [_vp, _i, C.POINTER(MotionState)]),
    "ov2_btracker_set_keyframe_info": (_i, [_vp, _i, _i, _d, _i]),
    "ov2_btracker_track_mono_begin": (_i, [_vp, _i, _vp, _i, _vp, _vp, _vp, _vp, _i, C.POINTER(TrackMonoParams), C.POINTER(TrackMonoInput)]),
    "ov2_btracker_track_mono_end": (_i, [_vp, _vp, _vp, _vp, C.POINTER(EpifilterResult), C.POINTER(PoseResult), C.POINTER(TrackMonoResult)]),
    "ov2_btracker_track_mono": (_i, [_vp, _i, _vp, _i, _vp, _vp, _vp, _vp, _i, C.POINTER(TrackMonoParams), C.POINTER(TrackMonoInput),
                                     _vp, _vp, _vp, C.POINTER(EpifilterResult), C.POINTER(PoseResult), C.POINTER(TrackMonoResult)]),
    "ov2_btracker_create_keyframe_begin": (_i, [_vp, _i, C.POINTER(CreateKeyframeParams), C.POINTER(CreateKeyframeInput)]),
    "ov2_btracker_create_keyframe_end": (_i, [_vp, C.POINTER(CreateKeyframeResult), _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "ov2_btracker_create_keyframe": (_i, [_vp, _i, C.POINTER(CreateKeyframeParams), C.POINTER(CreateKeyframeInput),
                                          C.POINTER(CreateKeyframeResult), _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "ov2_btracker_set_frame": (_i, [_vp, _i, _i, _vp, _vp, _vp, _vp]),
    "ov2_btracker_get_frame": (_i, [_vp, _i, _i, C.POINTER(_i), _vp, _vp, _vp, _vp]),
    "ov2_btracker_update_frame": (_i, [_vp, _i, _i, C.POINTER(ResidentOp), C.POINTER(ResidentUpdateResult)]),
    "ov2_btracker_update_frame_batch": (_i, [_vp, _i, C.POINTER(_i), C.POINTER(C.POINTER(ResidentOp)), C.POINTER(ResidentUpdateResult)]),
    "ov2_btracker_track_mono_resident_begin": (_i, [_vp, _i, _vp, _i, _i, C.POINTER(TrackMonoParams), C.POINTER(TrackMonoInput)]),
    "ov2_btracker_track_mono_resident_end": (_i, [_vp, _vp, _vp, _vp, C.POINTER(EpifilterResult), C.POINTER(PoseResult),
                                                  C.POINTER(TrackMonoResult), C.POINTER(ResidentStepResult)]),
    "ov2_btracker_track_mono_resident": (_i, [_vp, _i, _vp, _i, _i, C.POINTER(TrackMonoParams), C.POINTER(TrackMonoInput), _vp, _vp, _vp,
                                              C.POINTER(EpifilterResult), C.POINTER(PoseResult), C.POINTER(TrackMonoResult),
                                              C.POINTER(ResidentStepResult)]),
    "ov2_btracker_last_slot_bytes": (_i, [_vp, C.POINTER(C.c_size_t)]),
    "ov2_btracker_stereo_keyframe_begin": (_i, [_vp, _i, C.POINTER(StereoKeyframeParams), _vp, _vp]),
    "ov2_btracker_stereo_keyframe_end": (_i, [_vp, C.POINTER(StereoKeyframeResult), _vp, _vp, _vp, _vp, _vp]),
    "ov2_btracker_stereo_keyframe": (_i, [_vp, _i, C.POINTER(StereoKeyframeParams), _vp, _vp, C.POINTER(StereoKeyframeResult),
                                          _vp, _vp, _vp, _vp, _vp]),
    "ov2_btracker_get_keyframe_info": (_i, [_vp, _i, _i, C.POINTER(_i), C.POINTER(_d), C.POINTER(_i), C.POINTER(_i)]),
    "ov2_btracker_reserve_anchors": (_i, [_vp, _i]),
    "ov2_btracker_set_anchors": (_i, [_vp, _i, _i, _vp, _vp, _vp, _vp, _i, _vp, _vp]),
    "ov2_btracker_get_anchors": (_i, [_vp, _i, _i, C.POINTER(_i), _vp, _vp, _vp, _vp, C.POINTER(_i), _vp, _vp, _vp]),
    "ov2_btracker_set_anchor_poses_batch": (_i, [_vp, _i, _vp, _vp, _vp, C.POINTER(_i)]),
    "ov2_btracker_set_anchor_poses": (_i, [_vp, _i, _i, _vp, _vp, C.POINTER(_i)]),
    "ov2_btracker_temporal_keyframe_begin": (_i, [_vp, _i, C.POINTER(TemporalKeyframeParams), _vp]),
    "ov2_btracker_temporal_keyframe_end": (_i, [_vp, C.POINTER(TemporalKeyframeResult), _vp, _vp, _vp, _vp]),
    "ov2_btracker_temporal_keyframe": (_i, [_vp, _i, C.POINTER(TemporalKeyframeParams), _vp, C.POINTER(TemporalKeyframeResult),
                                            _vp, _vp, _vp, _vp]),
    "ov2_pyr_item_bytes": (C.c_size_t, [_vp]),
    "ov2_pyr_download_item": (_i, [_vp, _vp, _i, _vp]),
    "ov2_btracker_set_track_from_keyframe": (_i, [_vp, _i]),
    "ov2_btracker_adopt_keyframe_pyramid": (_i, [_vp, _i, _vp]),
    "ov2_btracker_set_keyframe_px": (_i, [_vp, _i, _i, _vp, _vp]),
    "ov2_btracker_get_keyframe_px": (_i, [_vp, _i, _i, C.POINTER(_i), _vp, _vp]),
    "ov2_btracker_kf_item": (_vp, [_vp, _i]),
}

OV2_ABI_VERSION = 600          # include/ov2slam_hip.h

_lib = None


def load():
    """Load libov2slam_hip.so and bind every symbol.  Fails loudly."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "%s is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C ov2slam_amd/csrc` (hipcc --offload-arch=gfx950).  There is no CPU fallback." % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError if the .so does not export it
        fn.restype = res
        fn.argtypes = args
    if lib.ov2_version() != OV2_ABI_VERSION:    # struct layouts below are those of include/ov2slam_hip.h at this version
        raise ImportError("%s reports ABI version %d, these bindings were written for %d: rebuild the library"
                          % (LIB_PATH, lib.ov2_version(), OV2_ABI_VERSION))
    _lib = lib
    return lib


def check(rc):
    if rc != OV2_OK:
        raise Ov2Error(rc, load().ov2_last_error().decode("utf-8", "replace"))
