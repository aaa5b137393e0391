// multi_view_geometry.hpp -- C++ adapter for MultiViewGeometry::ceresPnP (/root/reference/src/multi_view_geometry.cpp:492-586), the
// motion-only BA the front end runs per frame (src/visual_front_end.cpp:788-801) and the loop closer per candidate
// (src/loop_closer.cpp:882): ONE pose, ReprojectionErrorSE3 factors with fixed world points (OV2_RES_PNP), DENSE_QR in the
// reference, the same two-pass protocol:
//   pass 1    Huber(sqrt(chi2th)) if buse_robust, nmaxiter iterations, function_tolerance 1e-3, 5 ms time limit    (:519-544)
//   outliers  chi2err_ > chi2th or depth <= 0 on the values cached by the last Evaluate; their residual blocks are
//             removed when bapply_l2_after_robust; false when every observation is bad                            (:547-565)
//   pass 2    loss reset to L2, same options, only if bapply_l2_after_robust and outliers were found               (:567-570)
// The reference function is static and is called from two threads: the caller passes the context of ITS thread
// (ov2::SlamGpu::threadContext()).
//
// ov2::p3pRansac -- MultiViewGeometry::p3pRansac in its USE_OPENGV form (:144-343): Kneip's P3P under OpenGV's LMedS (the front end,
// src/visual_front_end.cpp:729-742) or RANSAC loop (the loop closer, src/loop_closer.cpp:817) on the device (ov2_p3p_ransac,
// csrc/p3p.hip).  OpenGV's solver and loops are restated, not linked: same algorithm, another random stream (see below).
//
// ov2::compute5ptEssentialMatrix -- MultiViewGeometry::compute5ptEssentialMatrix in its USE_OPENGV form (:594-696): Nister's five-point
// solver under OpenGV's RANSAC loop (the epipolar filter of the front end, src/visual_front_end.cpp:440-660, the initialisation, :946,
// and the loop closer, src/loop_closer.cpp:483) on the device (ov2_epipolar_ransac, csrc/fivept.hip).  Restated like the P3P search,
// not pinned against an OpenGV binary.
#pragma once
#include <algorithm>
#include <cmath>
#include "ov2_types.hpp"

namespace ov2 {

// vunkps: n x (u, v) undistorted pixels; vwpts: n x (x, y, z) world points; vscales: n pyramid scales (sigma = 2^scale);
// Twc: [tx ty tz qx qy qz qw], in / out (left unchanged when the function returns false before pass 2, like the reference's early return).
// max_solver_time_s: the reference's 0.005; <= 0 = no limit (results then do not depend on machine load).
// *error (may be NULL) receives the library's message when a solve could not run (the caller then falls back to Ceres).
inline bool ceresPnP(Context &ctx, const double *vunkps, const double *vwpts, const int *vscales, size_t n, double Twc[7], int nmaxiter,
                     float chi2th, bool buse_robust, bool bapply_l2_after_robust, float fx, float fy, float cx, float cy,
                     std::vector<int> &voutliersidx, double max_solver_time_s = 0.005, bool *library_ok = nullptr, std::string *error = nullptr)
{
    if (library_ok) *library_ok = true;
    if (n == 0) return false;
    std::vector<uint8_t> rtype(n, (uint8_t)OV2_RES_PNP), active(n, 1), dpos(n, 1), kfc(1, 0);
    std::vector<int> rkf(n, 0), rlm(n, -1);
    std::vector<double> sigma(n), chi2(n, 0.0);
    for (size_t i = 0; i < n; i++) sigma[i] = std::pow(2., vscales ? vscales[i] : 0);
    ov2_ba_problem p{};
    double pose[7];
    for (int i = 0; i < 7; i++) pose[i] = Twc[i];
    p.n_kf = 1; p.poses = pose; p.kf_const = kfc.data();
    p.n_lm = 0;
    p.n_res = (int)n; p.res_type = rtype.data(); p.res_kf = rkf.data(); p.res_lm = rlm.data(); p.res_uv = vunkps; p.res_sigma = sigma.data();
    p.res_xyz = vwpts; p.res_active = nullptr;
    p.calib_l[0] = fx; p.calib_l[1] = fy; p.calib_l[2] = cx; p.calib_l[3] = cy;
    for (int i = 0; i < 4; i++) p.calib_r[i] = p.calib_l[i];
    p.T_rl[6] = 1.0;
    ov2_ba_options o; ov2_ba_default_options(&o);
    o.max_iter = nmaxiter; o.function_tolerance = 1e-3; o.huber_delta = buse_robust ? std::sqrt((double)chi2th) : -1.0;
    o.max_solver_time_s = max_solver_time_s;
    double pose_out[7];
    ov2_ba_result r{};
    r.poses_out = pose_out; r.chi2_last_eval = chi2.data(); r.depthpos_last_eval = dpos.data();
    if (ov2_ba_solve(ctx.get(), &p, &o, &r) != OV2_OK) {
        if (library_ok) *library_ok = false;
        if (error) *error = ov2_last_error();
        return false;
    }
    size_t nbbad = 0;
    for (size_t i = 0; i < n; i++)
        if (chi2[i] > (double)chi2th || !dpos[i]) {                                            // :547-560
            if (bapply_l2_after_robust) active[i] = 0;
            voutliersidx.push_back((int)i);
            nbbad++;
        }
    if (nbbad == n) return false;                                                              // :562-564 (Twc untouched)
    int termination = r.termination;
    if (bapply_l2_after_robust && !voutliersidx.empty()) {                                     // :567-570
        for (int i = 0; i < 7; i++) pose[i] = pose_out[i];
        p.res_active = active.data();
        o.huber_delta = -1.0;
        if (ov2_ba_solve(ctx.get(), &p, &o, &r) != OV2_OK) {
            if (library_ok) *library_ok = false;
            if (error) *error = ov2_last_error();
            return false;
        }
        termination = r.termination;
    }
    for (int i = 0; i < 7; i++) Twc[i] = pose_out[i];                                           // :572
    return termination != OV2_TERM_FAILURE;                                                    // Summary::IsSolutionUsable (:574)
}

// ceresPnP's whole protocol in ONE launch (ov2_ceres_pnp, csrc/pnp.hip): one upload, one kernel, one download, one synchronisation
// instead of the two blocking solves above, and sums formed in a fixed order (the same bits in every run).  Arguments as ceresPnP;
// Twc is written whenever the library ran, also on a false return (the pose of pass 1 when every observation is bad).  There is
// no time limit.  ceresPnP above keeps its route through ov2_ba_solve.
inline bool ceresPnPFused(Context &ctx, const double *vunkps, const double *vwpts, const int *vscales, size_t n, double Twc[7], int nmaxiter,
                          float chi2th, bool buse_robust, bool bapply_l2_after_robust, float fx, float fy, float cx, float cy,
                          std::vector<int> &voutliersidx, bool *library_ok = nullptr, std::string *error = nullptr,
                          ov2_pnp_result *summary = nullptr)
{
    if (library_ok) *library_ok = true;
    if (n == 0) return false;
    const std::vector<int> zeros(vscales ? 0 : n, 0);
    std::vector<int> outliers(n);
    ov2_pnp_params P{};
    P.nmaxiter = nmaxiter; P.chi2th = (double)chi2th; P.use_robust = buse_robust ? 1 : 0; P.apply_l2_after_robust = bapply_l2_after_robust ? 1 : 0;
    P.K[0] = fx; P.K[1] = fy; P.K[2] = cx; P.K[3] = cy;
    ov2_pnp_problem pb{};
    pb.n = (int)n; pb.unpx = vunkps; pb.wpt = vwpts; pb.scale = vscales ? vscales : zeros.data(); pb.Twc = Twc;
    ov2_pnp_result r{};
    r.outliers = outliers.data();
    if (n > 0x7fffffffu || ov2_ceres_pnp(ctx.get(), &P, &pb, &r) != OV2_OK) {
        if (library_ok) *library_ok = false;
        if (error) *error = ov2_last_error();
        return false;
    }
    voutliersidx.insert(voutliersidx.end(), outliers.begin(), outliers.begin() + r.n_outliers);
    for (int i = 0; i < 7; i++) Twc[i] = r.Twc[i];
    if (summary) { *summary = r; summary->outliers = nullptr; }
    return r.success != 0;
}

// bvs / vwpts: n x 3 unit bearing vectors (camera frame) and world points.  Twc: [tx ty tz qx qy qz qw], written only when the
// function returns true (translation = the model's last column, rotation through Sophus::SE3d::setRotationMatrix: Eigen's
// Quaterniond(R), normalised).  voutliersidx receives every index that is not an inlier, ascending, only when the function returns
// true -- the reference returns before it touches either on its false paths (n < 4, fewer than 5 inliers, rotation not orthogonal).
// seed: the sample table is drawn from it (ov2_p3p_draw_samples, 2 x nmaxiter rows so that skipped rows do not shorten the
// search, at most OV2_P3P_MAX_ROWS), so a call is a deterministic function of its arguments; the reference draws from rand(), seeded
// by the clock when bdorandom -- which the shipped parameter files set -- so its own result differs from run to run.  bdorandom is
// accepted for the signature and not read: pass a varying seed for the same effect.
// boptimize (OpenGV's non-linear refinement on the inliers) is not provided: the call fails (*library_ok = false).  Refine the pose
// with ov2::ceresPnP, as LoopCloser::computePnP does right after.
inline bool p3pRansac(Context &ctx, const double *bvs, const double *vwpts, size_t n, int nmaxiter, float errth, bool boptimize,
                      bool bdorandom, float fx, float fy, double Twc[7], std::vector<int> &voutliersidx, bool use_lmeds,
                      unsigned long long seed, bool *library_ok = nullptr, std::string *error = nullptr)
{
    (void)bdorandom;
    if (library_ok) *library_ok = true;
    if (n < 4) return false;                                                                   // :178-180
    float focal = fx + fy;                                                                     // :209-213
    focal /= 2.;
    // The reference writes (1.0 - cos(atan(errth/focal))) with unqualified names: a build whose headers bring std::cos / std::atan
    // into scope resolves the float overloads (the threshold is then a float difference), one that sees only C's ::cos / ::atan
    // evaluates in double.  This adapter evaluates in double.
    ov2_p3p_params P{};
    P.mode = use_lmeds ? OV2_P3P_LMEDS : OV2_P3P_RANSAC;
    P.max_iterations = nmaxiter;
    P.threshold = 1.0 - std::cos(std::atan((double)(errth / focal)));
    P.probability = 0.99;
    P.boptimize = boptimize ? 1 : 0;
    const int rows = (int)std::min<long long>(2LL * std::max(nmaxiter, 0), OV2_P3P_MAX_ROWS);
    std::vector<int> samples(4 * (size_t)rows), outliers(n);
    ov2_p3p_problem pb{};
    pb.n = (int)n; pb.bv = bvs; pb.X = vwpts; pb.n_rows = rows; pb.samples = samples.data();
    ov2_p3p_result r{};
    r.outliers = outliers.data();
    if (ov2_p3p_draw_samples(seed, (int)n, rows, samples.data()) != OV2_OK || ov2_p3p_ransac(ctx.get(), &P, &pb, &r) != OV2_OK) {
        if (library_ok) *library_ok = false;
        if (error) *error = ov2_last_error();
        return false;
    }
    if (r.status != 0) return false;                                                           // :220-226
    const double *m = r.model;                                                                 // Rwc row-major, twc
    double q[4];                                                                               // x y z w: Eigen::Quaterniond(R)
    double t = m[0] + m[4] + m[8];
    if (t > 0.) {
        t = std::sqrt(t + 1.0);
        q[3] = 0.5 * t;
        t = 0.5 / t;
        q[0] = (m[7] - m[5]) * t; q[1] = (m[2] - m[6]) * t; q[2] = (m[3] - m[1]) * t;
    } else {
        int i = 0;
        if (m[4] > m[0]) i = 1;
        if (m[8] > m[4 * i]) i = 2;
        const int j = (i + 1) % 3, k = (j + 1) % 3;
        t = std::sqrt(m[4 * i] - m[4 * j] - m[4 * k] + 1.0);
        q[i] = 0.5 * t;
        t = 0.5 / t;
        q[3] = (m[3 * k + j] - m[3 * j + k]) * t;
        q[j] = (m[3 * j + i] + m[3 * i + j]) * t;
        q[k] = (m[3 * k + i] + m[3 * i + k]) * t;
    }
    const double qn = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);         // SO3::setQuaternion normalises
    Twc[0] = m[9]; Twc[1] = m[10]; Twc[2] = m[11];
    for (int i = 0; i < 4; i++) Twc[3 + i] = q[i] / qn;
    voutliersidx.reserve(n);                                                                   // :241-251
    voutliersidx.insert(voutliersidx.end(), outliers.begin(), outliers.begin() + r.n_outliers);
    return true;
}

// bvs1 / bvs2: n x 3 unit bearing vectors of the keyframe and of the current frame.  Rwc (row-major 3 x 3), twc and voutliersidx are
// written only when the function returns true, as the reference returns before it touches them on its false paths (n < 8, fewer
// than 10 inliers).  The model is x1 = Rwc x2 + twc with |twc| = 1.
// bdorandom selects the seed policy of the sample table (ov2_epipolar_draw_samples, 2 x nmaxiter rows so that skipped rows do not
// shorten the search, at most OV2_EPI_MAX_ROWS): false = the fixed seed 0, so that two calls on the same matches agree, as OpenGV's
// constant srand does; true = the caller's `seed`, which the caller varies, standing in for OpenGV's clock-seeded rand().
// boptimize (OpenGV's non-linear refinement on the inliers; the front end asks for it only in the mono branch when tracking is
// poor) is not provided: the call fails (*library_ok = false).
inline bool compute5ptEssentialMatrix(Context &ctx, const double *bvs1, const double *bvs2, size_t n, int nmaxiter, float errth,
                                      bool boptimize, bool bdorandom, float fx, float fy, double Rwc[9], double twc[3],
                                      std::vector<int> &voutliersidx, unsigned long long seed = 0, bool *library_ok = nullptr,
                                      std::string *error = nullptr)
{
    if (library_ok) *library_ok = true;
    if (n < 8) return false;                                                                   // :624-626
    float focal = fx + fy;                                                                     // :654-658
    focal /= 2.;
    ov2_epipolar_params P{};
    P.max_iterations = nmaxiter;
    P.threshold = 2.0 * (1.0 - std::cos(std::atan((double)(errth / focal))));
    P.probability = 0.99;
    P.boptimize = boptimize ? 1 : 0;
    const int rows = (int)std::min<long long>(2LL * std::max(nmaxiter, 0), OV2_EPI_MAX_ROWS);
    std::vector<int> samples(8 * (size_t)rows), outliers(n);
    ov2_epipolar_problem pb{};
    pb.n = (int)n; pb.bv1 = bvs1; pb.bv2 = bvs2; pb.n_rows = rows; pb.samples = samples.data();
    ov2_epipolar_result r{};
    r.outliers = outliers.data();
    if (ov2_epipolar_draw_samples(bdorandom ? seed : 0ull, (int)n, rows, samples.data()) != OV2_OK ||
        ov2_epipolar_ransac(ctx.get(), &P, &pb, &r) != OV2_OK) {
        if (library_ok) *library_ok = false;
        if (error) *error = ov2_last_error();
        return false;
    }
    if (r.status != 0) return false;                                                           // :665-667
    for (int i = 0; i < 9; i++) Rwc[i] = r.model[i];                                            // :669-670
    for (int i = 0; i < 3; i++) twc[i] = r.model[9 + i];
    voutliersidx.reserve(n);                                                                   // :683-693
    voutliersidx.insert(voutliersidx.end(), outliers.begin(), outliers.begin() + r.n_outliers);
    return true;
}

}  // namespace ov2
