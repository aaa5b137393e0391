// ba.hip -- anchored-inverse-depth local bundle adjustment on gfx950 (fp64).
//
// Replaces the two ceres::Solve calls of Optimizer::localBA
// (/root/reference/src/optimizer.cpp:479 robust pass, :618 L2 pass) together with the factor
// arithmetic of src/ceres_parametrization.cpp:361-712 and Ceres 2.0.0's trust-region
// Levenberg-Marquardt + Schur-complement machinery (trust_region_minimizer.cc,
// levenberg_marquardt_strategy.cc, schur_eliminator_impl.h, corrector.cc, loss_function.cc).
//
// Device-side design
//   * The whole LM loop runs on the GPU: every kernel reads a control block (BACtl) in HBM and
//     returns at once when the solver has terminated or its phase is not needed, so the host
//     enqueues a fixed kernel sequence for max_iter iterations and synchronises ONCE.
//   * Linearisation (k_ba_linearize): one wavefront per landmark, one lane per residual block.
//     Per-residual 2x6 / 2x6 / 2x1 Jacobians are built in registers, robustified (Huber +
//     Ceres corrector) and immediately contracted: the landmark's E-side sums (E^T E, E^T b and
//     its dense row of W = E^T F) are reduced inside the wave (shuffles / an LDS row) and written
//     once, coalesced; pose-side blocks (F^T F, F^T b) are accumulated with fp64 atomics.
//     No Jacobian is ever materialised in HBM.
//   * The normal equations are kept UNSCALED; Jacobi scaling s, the LM diagonal D and the trust
//     region radius enter algebraically per iteration:
//         S  = s_i s_j (H_ij - sum_l W_li c_l W_lj) + delta_ij D_i^2,  c_l = s_l^2 / (s_l^2 ete_l + D_l^2)
//     so a rejected step re-runs only the W^T C W contraction (k_ba_schur_gemm, LDS-tiled,
//     split over landmarks), the dense Cholesky (k_ba_cholesky, one workgroup) and the
//     back-substitution -- not the Jacobians.
//   * Step acceptance, radius update, tolerances and the "last evaluated point" bookkeeping
//     (chi2err_/isdepthpositive_ caching) follow Ceres exactly (k_ba_iter_begin,
//     k_ba_candidate, k_ba_decide).
#include "common.hpp"
#include <math.h>
#include <float.h>
#include <algorithm>
#include <stdlib.h>
#include <vector>
#include <atomic>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <chrono>
#include <thread>

#pragma clang fp contract(fast)   // BA parity is 1e-4 relative in fp64: FMA contraction is fine here

#define BA_TILE 32
#define BA_MAX_NFP 6144     // 1024 optimised keyframes: H, G, S are dense nfp x nfp doubles (302 MB each at the cap)

#define BA_PART_MAX 2048
#define BA_TRACE_CAP 64
typedef ov2_ba_iter BAIterRec;   // the iteration summary Ceres pushes into Solver::Summary::iterations (OV2_OPT_BA_TRACE)
struct BACtl {
    // accumulators
    double cost_acc;
    double acc1, acc2, acc3;      // sum_l y_l g'_l ; sum_l (2 y_l s_l t_l + s_l^2 ete_l y_l^2) ; sum_l c_l t_l^2
    double acc_sn, acc_xn;        // landmark part of |x - candidate|^2 and |candidate|^2 (k_ba_backsub, inverse-depth form)
    int bad_step;                 // a non-finite landmark step (k_ba_backsub)
    int reuse_now;                // reuse_diag as this iteration found it (k_ba_iter_begin sets reuse_diag = 1 when it is done)
    unsigned long long dbg[8];    // phase clocks of the last k_ba_cholesky (wall_clock64 ticks)
    // LM / TR state
    double radius, decrease_factor;
    double x_cost, cand_cost, model_cost_change, x_norm, minimum_cost, initial_cost, gmax;
    double ev_min, ev_cur, ev_ref, ev_cand, ev_acc_ref, ev_acc_cand;
    int ev_nonmono;
    int reuse_diag;
    int iteration, n_steps, n_success, num_invalid, termination, done;
    int need_lin, fresh_lin, step_successful, step_valid, lin_fail, scaled;
    // OV2_OPT_BA_TRACE: the summary of the iteration under way and where finished ones go (NULL: no trace)
    BAIterRec cur;
    BAIterRec *trace;
    int n_trace;
};

struct BADev {                    // device pointers + sizes (passed by value to kernels)
    int n_kf, n_lm, n_act, nf, nfp;
    int *flag_h;                  // pinned host word: 2 * (iteration whose outcome is known) + done, written by k_ba_decide
    // inverse-depth form: per-work-group partial sums of k_ba_backsub (rows 0-4: acc1, acc2, acc3, step norm, candidate norm) and
    // k_ba_cost (row 5), BA_PART_MAX entries each, summed by the one-work-group kernel that consumes them -- a global atomic per
    // work-group on five words of the control block was most of those kernels' time (the same addresses, one L2 channel)
    double *part; int bs_blocks, cost_blocks, lin_blocks;
    double min_diag, max_diag;    // clamp of the LM diagonal (BAOpt), for the kernels that form c_l themselves (d_lm_c)
    // OV2_OPT_BA_DETERMINISTIC: the linearisers (one wavefront per work-group) add into their OWN copy of H / F^T b (Hpart / bfpart,
    // det_lin + det_po copies) and store their cost in costpart; k_ba_det_reduce adds the copies up in a fixed order.  k_ba_schur_gemm
    // stores the tiles of each landmark split (Gpart / vpart, det_ksplit copies); k_ba_assemble adds them up in order.
    int det, det_lin, det_po, det_ksplit;
    double *Hpart, *bfpart, *costpart, *Gpart, *vpart;
    // ldim = 1: anchored inverse depth (one scalar per landmark); ldim = 3: 3-D point landmarks with variable poses
    // (buse_inv_depth: 0, optimizer.cpp:207-209 / :333-384).  Per-landmark state arrays (x_lam, c_lam, scale_l, diag_l, etb,
    // yl) hold ldim entries per landmark, W holds ldim rows per landmark; the 3x3 e-block data is in ete6 / minv6.
    int ldim;
    // big = 1: more optimised keyframes than the LDS-resident path holds (~90).  W = E^T F is then kept SPARSE: one 6-double
    // "slot" per (landmark, optimised keyframe that sees or anchors it) in cww -- the anchor block and the left / right observer
    // blocks of one keyframe share a slot -- instead of a dense n_lm x nfp matrix.  The anchor-observer blocks of H go to HBM with
    // global atomics, the Schur complement is accumulated row block by row block in LDS from per-keyframe slot lists
    // (k_ba_schur_sparse) and the reduced system is factored by a multi-kernel blocked Cholesky on HBM (k_chol_*).
    int big, n_cw;
    int chol_hbm;                 // reduced system factored by the multi-kernel Cholesky on HBM (k_chol_*): always with big, and for 3-D point
                                  // problems (dense W, k_ba_schur_gemm) whose reduced system outgrows the one-work-group LDS kernel
    int lin_waves;                // 3-D point lineariser: wavefronts per work-group (each keeps 3 rows of W in LDS: 4 up to ~200 keyframes, 2, 1 up to ~450)
    int lin_direct;               // big path with more optimised keyframes than the work-group's LDS can pre-aggregate (n_opt x 27 doubles:
                                  // ~570): observer diagonal blocks and F^T b go to H / bf with global atomics as well
    double *cww;                  // 6*n_cw   slot values (zeroed by k_ba_zero_lin, filled by the lineariser)          [big]
    int *cw_ptr;                  // n_lm+1   slots of a landmark                                                      [big]
    int *cw_col;                  // n_cw     pose column of the slot
    int *cw_lm;                   // n_cw     landmark of the slot
    int *res_cw;                  // n_act    slot of the residual block's observer (-1: constant observer / right-anchor block)
    int *lm_cwa;                  // n_lm     slot of the landmark's anchor (-1: constant anchor or no residual blocks)
    int *kfl_ptr, *kfl_idx;       // n_opt+1, n_cw : slots by optimised keyframe
    double *ete6;                 // 6*n_lm   unscaled E^T E, upper triangle (xx xy xz yy yz zz)            [ldim 3]
    double *minv6;                // 6*n_lm   (S E^T E S + D^2)^-1, upper triangle                          [ldim 3]
    double *Wp;                   // 3*n_lm * nfp : rows L_c^T W_l with C_l = S M^-1 S = L_c L_c^T, so that
                                  //   sum_l W_l^T C_l W_l = Wp^T Wp  -- k_ba_schur_gemm runs on it unchanged   [ldim 3]
    double *ep;                   // 3*n_lm   L_c^T E^T b                                                    [ldim 3]
    double *ones;                 // 3*n_lm   the "c_l" of the pseudo-rows of Wp                              [ldim 3]
    // problem (landmark-sorted residuals)
    const int *pose_col;          // n_kf  (-1 = constant)
    const int *lm_ptr;            // n_lm+1
    const int *lm_anchor;         // n_lm
    const double *lm_auv;         // 2*n_lm
    const uint8_t *res_type;      // n_act
    const int *res_kf;            // n_act
    const int *res_orig;          // n_act -> index in the caller's arrays
    const double *res_uv;         // 2*n_act
    const double *res_sigma;      // n_act
    // pose-only residual blocks (OV2_RES_PNP), not attached to a landmark
    int n_po;
    const int *po_kf, *po_orig;   // n_po
    const double *po_xyz, *po_uv, *po_sigma;   // 3, 2, 1 per block
    double calib_l[4], calib_r[4];
    double Rrl[9], trl[3];
    double huber;                 // <= 0 : trivial loss
    // state
    double *x_pose, *c_pose;      // 7*n_kf
    double *x_RT, *c_RT;          // 12*n_kf : Rwc row-major (9) + t (3)
    double *x_lam, *c_lam;        // n_lm
    double *scale_f, *diag_f;     // nfp
    double *scale_l, *diag_l;     // n_lm
    double *ete, *etb;            // n_lm  (unscaled E^T E, E^T b)
    double *cl, *ce;              // n_lm  c_l, c_l * etb_l
    double *W;                    // n_lm * nfp (unscaled E^T F)
    double *H, *G;                // nfp*nfp (unscaled F^T F ; W^T C W, upper tiles)
    double *bf, *v;               // nfp  (unscaled F^T b ; W^T (c etb))
    double *S;                    // nfp*nfp scratch for the Cholesky
    double *Linv;                 // nfp*32: inverse 32x32 diagonal blocks of the factor
    double *yf;                   // nfp
    double *yl;                   // n_lm
    double *chi2;                 // n_res (caller order)
    uint8_t *dpos;                // n_res
    // resident two-pass localBA (ov2_local_ba): residual blocks are deactivated ON THE DEVICE between the passes
    uint8_t *res_off;             // n_act (landmark-sorted order): 1 = removed from the problem (optimizer.cpp:500-592)   [ldim 1]
    uint8_t *lm_live;             // n_lm : the landmark still has a residual block (a block-less landmark is not part of
                                  //        the program, program.cc RemoveFixedBlocks); NULL = derive it from lm_ptr
    uint8_t *bad_obs;             // n_res (caller order): outlier verdicts of k_ba_mark_outliers
    int *lba_cnt;                 // 8 counters of k_ba_mark_outliers
    BACtl *ctl;
    // lock-step batch of problems (ov2_local_ba_batch: one launch per kernel, blockIdx.z = problem): what the single-problem launches
    // pass as kernel arguments or decide on the host, per problem
    int g_ntiles, g_nupper, g_lmps, g_ksplit;     // k_ba_schur_gemm's tile count / upper tiles / landmarks per split / splits
    const int *lm_order_b;                        // the lineariser's anchor-sorted landmark order
    const double *pose0, *lam0;                   // the problem's initial parameters (7 n_kf, n_lm)
    int n_res;                                    // residual blocks of the caller's arrays (chi2 / dpos / bad_obs entries)
    uint8_t *out_b; int out_flags;                // the problem's slot of the batch's result block (k_ba_gather_B); 1: + chi2, 2: + depth flags
    int skip2;                                    // the problem takes no second pass (no outliers / stop requested): its second outlier test is skipped
};

__device__ __forceinline__ bool d_lm_has(const BADev &D, int lm)
{
    return D.lm_live ? D.lm_live[lm] != 0 : D.lm_ptr[lm] != D.lm_ptr[lm + 1];
}

// c_l = s^2 / (s^2 E^T E + D_l^2 / radius) of an inverse-depth landmark (0 without live blocks), D_l^2 = the clamped diagonal of the
// scaled E^T E -- kept from the last iteration that did not reuse it (LevenbergMarquardtStrategy).  Formed by its consumers
// (k_ba_schur_gemm, k_ba_backsub) since round 4: k_ba_iter_begin used to walk the landmarks with one work-group for it.
__device__ __forceinline__ double d_lm_c(const BADev &D, int l, double radius, int reuse, double *dg_out = nullptr)
{
    if (!d_lm_has(D, l)) return 0.0;
    const double s = D.scale_l[l], e = D.ete[l];
    const double dg = reuse ? D.diag_l[l] : fmin(fmax(s * s * e, D.min_diag), D.max_diag);
    if (dg_out) *dg_out = dg;
    return s * s / (s * s * e + dg / radius);
}

struct BAOpt {
    int max_iter;
    double ftol, gtol, ptol, max_radius, min_radius, min_diag, max_diag, min_rel_decrease;
    int jacobi, max_invalid;
};

// ---------------------------------------------------------------------------------- trust-region bookkeeping (one thread)
// The three scalar state machines of Ceres' TrustRegionMinimizer as pure functions on the control block, shared by the
// multi-kernel solver (k_ba_iter_begin / k_ba_candidate / k_ba_decide) and the single-kernel pose-only solver (k_pnp_solve).
__device__ __forceinline__ void d_ctl_iter_begin(BACtl &cl, const BAOpt &O, int fresh, double gmax)
{
    BACtl *ctl = &cl;
    if (fresh) {
        ctl->gmax = gmax;
        ctl->x_cost = ctl->cost_acc;
        ctl->cost_acc = 0;
        if (!ctl->scaled) {             // iteration zero
            ctl->scaled = 1;
            ctl->initial_cost = ctl->x_cost; ctl->minimum_cost = ctl->x_cost;
            ctl->ev_min = ctl->ev_cur = ctl->ev_ref = ctl->ev_cand = ctl->x_cost;
            ctl->ev_acc_ref = ctl->ev_acc_cand = 0; ctl->ev_nonmono = 0;
        }
        ctl->fresh_lin = 0;
        ctl->reuse_diag = 0;
        // IterationZero / HandleSuccessfulStep -> EvaluateGradientAndJacobian: cost and gradient norm of the new point
        ctl->cur.cost = ctl->x_cost; ctl->cur.gradient_max_norm = gmax;
        if (ctl->cur.iteration == 0) { ctl->cur.step_is_valid = 1; ctl->cur.step_is_successful = 1; }
    }
    // FinalizeIterationAndCheckIfMinimizerCanContinue
    if (ctl->step_successful) {
        ctl->n_success++;
        if (ctl->x_cost < ctl->minimum_cost) ctl->minimum_cost = ctl->x_cost;
    }
    ctl->cur.trust_region_radius = ctl->radius;
    if (ctl->trace) { if (ctl->n_trace < BA_TRACE_CAP) ctl->trace[ctl->n_trace] = ctl->cur; ctl->n_trace++; }
    if (ctl->iteration >= O.max_iter) { ctl->termination = OV2_TERM_NO_CONVERGENCE; ctl->done = 1; }
    else if (ctl->step_successful && ctl->gmax <= O.gtol) { ctl->termination = OV2_TERM_GRADIENT_TOL; ctl->done = 1; }
    else if (ctl->radius <= O.min_radius) { ctl->termination = OV2_TERM_MIN_RADIUS; ctl->done = 1; }
    else {
        ctl->iteration++;
        ctl->step_successful = 0;
        ctl->step_valid = 0;
        ctl->lin_fail = 0;
        ctl->n_steps++;
        ctl->acc1 = 0; ctl->acc2 = 0; ctl->acc3 = 0; ctl->acc_sn = 0; ctl->acc_xn = 0; ctl->bad_step = 0;
        // the next summary: iteration number, the gradient norm of the last accepted point (trust_region_minimizer.cc:87-93, :124-126)
        ctl->cur.iteration = ctl->iteration; ctl->cur.step_is_valid = 0; ctl->cur.step_is_successful = 0;
        ctl->cur.cost = 0; ctl->cur.cost_change = 0; ctl->cur.step_norm = 0; ctl->cur.relative_decrease = 0;
    }
}

// returns 1 when the step is valid (model cost change > 0); P1 = y . g'_f, P2 = y^T H'_pp y of the pose part
__device__ __forceinline__ int d_ctl_candidate(BACtl &cl, const BAOpt &O, int ok, double P1, double P2)
{
    BACtl *ctl = &cl;
    int valid = 0;
    if (ok) {
        // model_cost_change = -(J step).(r + J step / 2) with step = -y  ==  y.g' - y^T H' y / 2
        const double mcc = (P1 + ctl->acc1) - 0.5 * (P2 + ctl->acc3 + ctl->acc2);
        ctl->model_cost_change = mcc;
        valid = mcc > 0.0;
    }
    if (!valid) {
        // HandleInvalidStep (trust_region_minimizer.cc:436-459)
        if (++ctl->num_invalid >= O.max_invalid) { ctl->termination = OV2_TERM_INVALID_STEPS; ctl->done = 1; }
        else { ctl->radius = ctl->radius / ctl->decrease_factor; ctl->decrease_factor *= 2.0; ctl->reuse_diag = 1; }
        ctl->step_valid = 0;
        ctl->cur.cost = ctl->x_cost;                       // "a step of length zero and no progress" (:476-484)
    } else {
        ctl->num_invalid = 0;
        ctl->step_valid = 1;
        ctl->cur.step_is_valid = 1;
    }
    return valid;
}

// returns 1 when the candidate is accepted; SN = |x - candidate|^2, XN = |candidate|^2 over the variable blocks
__device__ __forceinline__ int d_ctl_decide(BACtl &cl, const BAOpt &O, double SN, double XN)
{
    BACtl *ctl = &cl;
    int accept = 0;
    const double cand = ctl->cost_acc;
    ctl->cost_acc = 0;
    ctl->cand_cost = cand;
    ctl->cur.step_norm = sqrt(SN); ctl->cur.cost_change = ctl->x_cost - cand;
    if (sqrt(SN) <= O.ptol * (ctl->x_norm + O.ptol)) { ctl->termination = OV2_TERM_PARAMETER_TOL; ctl->done = 1; }
    else if (fabs(ctl->x_cost - cand) <= O.ftol * ctl->x_cost) { ctl->termination = OV2_TERM_FUNCTION_TOL; ctl->done = 1; }
    else {
        const double mcc = ctl->model_cost_change;
        const double r1 = (ctl->ev_cur - cand) / mcc, r2 = (ctl->ev_ref - cand) / (ctl->ev_acc_ref + mcc);
        const double rel = fmax(r1, r2);
        ctl->cur.relative_decrease = rel;
        if (rel > O.min_rel_decrease) {
            accept = 1;
            ctl->cur.step_is_successful = 1;               // (cost and gradient norm: the next k_ba_iter_begin, from the fresh linearisation)
            ctl->x_norm = sqrt(XN);
            ctl->step_successful = 1;
            ctl->need_lin = 1;
            // LevenbergMarquardtStrategy::StepAccepted
            const double t = 2.0 * rel - 1.0;
            ctl->radius = fmin(O.max_radius, ctl->radius / fmax(1.0 / 3.0, 1.0 - t * t * t));
            ctl->decrease_factor = 2.0; ctl->reuse_diag = 0;
            // TrustRegionStepEvaluator::StepAccepted (max_consecutive_nonmonotonic_steps = 0)
            ctl->ev_cur = cand; ctl->ev_acc_cand += mcc; ctl->ev_acc_ref += mcc;
            if (ctl->ev_cur < ctl->ev_min) { ctl->ev_min = ctl->ev_cur; ctl->ev_nonmono = 0; ctl->ev_cand = ctl->ev_cur; ctl->ev_acc_cand = 0; }
            else { ctl->ev_nonmono++; if (ctl->ev_cur > ctl->ev_cand) { ctl->ev_cand = ctl->ev_cur; ctl->ev_acc_cand = 0; } }
            if (ctl->ev_nonmono == 0) { ctl->ev_ref = ctl->ev_cand; ctl->ev_acc_ref = ctl->ev_acc_cand; }
        } else {
            ctl->radius = ctl->radius / ctl->decrease_factor; ctl->decrease_factor *= 2.0; ctl->reuse_diag = 1;
            ctl->cur.cost = cand;                          // the rejected candidate's cost (:119-127)
        }
    }
    return accept;
}

// ---------------------------------------------------------------------------------- algebra
__device__ __forceinline__ void d_quat_to_R(const double *q, double *R)
{
    double x = q[0], y = q[1], z = q[2], w = q[3];
    const double n = sqrt(x * x + y * y + z * z + w * w);
    x /= n; y /= n; z /= n; w /= n;
    const double tx = 2 * x, ty = 2 * y, tz = 2 * z;
    const double twx = tx * w, twy = ty * w, twz = tz * w, txx = tx * x, txy = ty * x, txz = tz * x;
    const double tyy = ty * y, tyz = tz * y, tzz = tz * z;
    R[0] = 1 - (tyy + tzz); R[1] = txy - twz;       R[2] = txz + twy;
    R[3] = txy + twz;       R[4] = 1 - (txx + tzz); R[5] = tyz - twx;
    R[6] = txz - twy;       R[7] = tyz + twx;       R[8] = 1 - (txx + tyy);
}

// T' = Exp(delta) * T   (se3left_parametrization.hpp:45-57, Sophus se3.hpp:763-784, so3.hpp:585-621)
__device__ void d_se3_left_plus(const double *pose, const double *a, double *out)
{
    const double *om = a + 3;
    const double theta_sq = om[0] * om[0] + om[1] * om[1] + om[2] * om[2];
    double theta, imag, real;
    if (theta_sq < 1e-10 * 1e-10) {
        theta = 0;
        const double t4 = theta_sq * theta_sq;
        imag = 0.5 - (1.0 / 48.0) * theta_sq + (1.0 / 3840.0) * t4;
        real = 1.0 - (1.0 / 8.0) * theta_sq + (1.0 / 384.0) * t4;
    } else {
        theta = sqrt(theta_sq);
        const double half = 0.5 * theta;
        imag = sin(half) / theta;
        real = cos(half);
    }
    const double qe[4] = {imag * om[0], imag * om[1], imag * om[2], real};
    double V[9], Re[9];
    d_quat_to_R(qe, Re);
    if (theta < 1e-10) {
        for (int k = 0; k < 9; k++) V[k] = Re[k];
    } else {
        const double O[9] = {0, -om[2], om[1], om[2], 0, -om[0], -om[1], om[0], 0};
        const double c1 = (1.0 - cos(theta)) / theta_sq, c2 = (theta - sin(theta)) / (theta_sq * theta);
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) {
                const double o2 = O[3 * i] * O[j] + O[3 * i + 1] * O[3 + j] + O[3 * i + 2] * O[6 + j];
                V[3 * i + j] = c1 * O[3 * i + j] + c2 * o2 + (i == j ? 1.0 : 0.0);
            }
    }
    double q[4] = {pose[3], pose[4], pose[5], pose[6]};
    const double qn = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    q[0] /= qn; q[1] /= qn; q[2] /= qn; q[3] /= qn;
    const double ax = qe[0], ay = qe[1], az = qe[2], aw = qe[3], bx = q[0], by = q[1], bz = q[2], bw = q[3];
    double r[4];
    r[3] = aw * bw - ax * bx - ay * by - az * bz;
    r[0] = aw * bx + ax * bw + ay * bz - az * by;
    r[1] = aw * by + ay * bw + az * bx - ax * bz;
    r[2] = aw * bz + az * bw + ax * by - ay * bx;
    const double rn = sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2] + r[3] * r[3]);
    for (int i = 0; i < 3; i++)
        out[i] = V[3 * i] * a[0] + V[3 * i + 1] * a[1] + V[3 * i + 2] * a[2] +
                 Re[3 * i] * pose[0] + Re[3 * i + 1] * pose[1] + Re[3 * i + 2] * pose[2];
    out[3] = r[0] / rn; out[4] = r[1] / rn; out[5] = r[2] / rn; out[6] = r[3] / rn;
}

__device__ __forceinline__ void d_pose_to_RT(const double *pose, double *RT)
{
    d_quat_to_R(pose + 3, RT);
    RT[9] = pose[0]; RT[10] = pose[1]; RT[11] = pose[2];
}

// Huber (loss_function.cc:48-62) -> (rho, rho')
__device__ __forceinline__ void d_huber(double a, double s, double &rho0, double &rho1)
{
    if (a > 0 && s > a * a) {
        const double r = sqrt(s);
        rho0 = 2.0 * a * r - a * a;
        rho1 = fmax(DBL_MIN, a / r);
    } else { rho0 = s; rho1 = 1.0; }
}

// One residual block.  RTa / RTo: anchor / observer (Rwc | t).  Returns the depth-positive flag.
// Jacobians are w.r.t. the left-multiplicative se(3) tangents [dt, dw] (2x6 row-major) and lambda.
template <bool JAC>
__device__ __forceinline__ int d_residual(const BADev &D, int type, const double *RTa, const double *RTo, double lam,
                                          const double *auv, const double *uv, double sigma,
                                          double *r, double *Ja, double *Jo, double *Jl)
{
    const double sqrt_info = 1.0 / sigma, zanch = 1.0 / lam;
    const double ap[3] = {zanch * ((auv[0] - D.calib_l[2]) / D.calib_l[0]), zanch * ((auv[1] - D.calib_l[3]) / D.calib_l[1]), zanch};
    const double *K = type == OV2_RES_LEFT ? D.calib_l : D.calib_r;
    double cam[3], wpt[3] = {0, 0, 0}, Ra[3] = {0, 0, 0};
    if (type == OV2_RES_RIGHT_ANCH) {
        for (int i = 0; i < 3; i++) cam[i] = D.Rrl[3 * i] * ap[0] + D.Rrl[3 * i + 1] * ap[1] + D.Rrl[3 * i + 2] * ap[2] + D.trl[i];
    } else {
        for (int i = 0; i < 3; i++) { Ra[i] = RTa[3 * i] * ap[0] + RTa[3 * i + 1] * ap[1] + RTa[3 * i + 2] * ap[2]; wpt[i] = Ra[i] + RTa[9 + i]; }
        const double d[3] = {wpt[0] - RTo[9], wpt[1] - RTo[10], wpt[2] - RTo[11]};
        double lc[3];
        for (int i = 0; i < 3; i++) lc[i] = RTo[i] * d[0] + RTo[3 + i] * d[1] + RTo[6 + i] * d[2];      // Rcw = Rwc^T
        if (type == OV2_RES_LEFT) { cam[0] = lc[0]; cam[1] = lc[1]; cam[2] = lc[2]; }
        else for (int i = 0; i < 3; i++) cam[i] = D.Rrl[3 * i] * lc[0] + D.Rrl[3 * i + 1] * lc[1] + D.Rrl[3 * i + 2] * lc[2] + D.trl[i];
    }
    const double invz = 1.0 / cam[2];
    r[0] = sqrt_info * (K[0] * cam[0] * invz + K[2] - uv[0]);
    r[1] = sqrt_info * (K[1] * cam[1] * invz + K[3] - uv[1]);
    const int dp = cam[2] > 0;
    if (!JAC) return dp;
    const double invz2 = invz * invz;
    const double Jc[6] = {invz * K[0], 0, -cam[0] * invz2 * K[0], 0, invz * K[1], -cam[1] * invz2 * K[1]};
    double M[9];
    if (type == OV2_RES_RIGHT_ANCH) { for (int k = 0; k < 9; k++) M[k] = D.Rrl[k]; }
    else if (type == OV2_RES_LEFT) { for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) M[3 * i + j] = RTo[3 * j + i]; }
    else for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++)
        M[3 * i + j] = D.Rrl[3 * i] * RTo[3 * j] + D.Rrl[3 * i + 1] * RTo[3 * j + 1] + D.Rrl[3 * i + 2] * RTo[3 * j + 2];   // Rrl * Rcw (Rcw = Rwc^T)
    double JR[6];
    for (int i = 0; i < 2; i++) for (int j = 0; j < 3; j++) JR[3 * i + j] = Jc[3 * i] * M[j] + Jc[3 * i + 1] * M[3 + j] + Jc[3 * i + 2] * M[6 + j];
    if (type == OV2_RES_RIGHT_ANCH) {
        for (int k = 0; k < 12; k++) { Ja[k] = 0; Jo[k] = 0; }
        const double jl[3] = {-zanch * ap[0], -zanch * ap[1], -zanch * ap[2]};
        Jl[0] = sqrt_info * (JR[0] * jl[0] + JR[1] * jl[1] + JR[2] * jl[2]);
        Jl[1] = sqrt_info * (JR[3] * jl[0] + JR[4] * jl[1] + JR[5] * jl[2]);
        return dp;
    }
    const double S[9] = {0, -wpt[2], wpt[1], wpt[2], 0, -wpt[0], -wpt[1], wpt[0], 0};
    for (int i = 0; i < 2; i++)
        for (int j = 0; j < 3; j++) {
            const double jrs = JR[3 * i] * S[j] + JR[3 * i + 1] * S[3 + j] + JR[3 * i + 2] * S[6 + j];
            Ja[6 * i + j] = sqrt_info * JR[3 * i + j];  Ja[6 * i + 3 + j] = -sqrt_info * jrs;
            Jo[6 * i + j] = -sqrt_info * JR[3 * i + j]; Jo[6 * i + 3 + j] = sqrt_info * jrs;
        }
    const double jl[3] = {-zanch * Ra[0], -zanch * Ra[1], -zanch * Ra[2]};
    Jl[0] = sqrt_info * (JR[0] * jl[0] + JR[1] * jl[1] + JR[2] * jl[2]);
    Jl[1] = sqrt_info * (JR[3] * jl[0] + JR[4] * jl[1] + JR[5] * jl[2]);
    return dp;
}

__device__ __forceinline__ void wave_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// DirectLeftSE3::ReprojectionErrorSE3 (ceres_parametrization.cpp:301-358): fixed world point, Jacobian w.r.t. the pose
template <bool JAC>
__device__ __forceinline__ int d_residual_pnp(const BADev &D, const double *RTo, const double *xyz, const double *uv, double sigma,
                                              double *r, double *Jo)
{
    const double sqrt_info = 1.0 / sigma;
    const double d[3] = {xyz[0] - RTo[9], xyz[1] - RTo[10], xyz[2] - RTo[11]};
    double c[3];
    for (int i = 0; i < 3; i++) c[i] = RTo[i] * d[0] + RTo[3 + i] * d[1] + RTo[6 + i] * d[2];      // Rcw = Rwc^T
    const double invz = 1.0 / c[2];
    const double *K = D.calib_l;
    r[0] = sqrt_info * (K[0] * c[0] * invz + K[2] - uv[0]);
    r[1] = sqrt_info * (K[1] * c[1] * invz + K[3] - uv[1]);
    if (JAC) {
        const double invz2 = invz * invz;
        const double Jc[6] = {invz * K[0], 0, -c[0] * invz2 * K[0], 0, invz * K[1], -c[1] * invz2 * K[1]};
        double JR[6];
        for (int i = 0; i < 2; i++) for (int j = 0; j < 3; j++) JR[3 * i + j] = Jc[3 * i] * RTo[3 * j] + Jc[3 * i + 1] * RTo[3 * j + 1] + Jc[3 * i + 2] * RTo[3 * j + 2];
        const double S[9] = {0, -xyz[2], xyz[1], xyz[2], 0, -xyz[0], -xyz[1], xyz[0], 0};
        for (int i = 0; i < 2; i++)
            for (int j = 0; j < 3; j++) {
                const double jrs = JR[3 * i] * S[j] + JR[3 * i + 1] * S[3 + j] + JR[3 * i + 2] * S[6 + j];
                Jo[6 * i + j] = -sqrt_info * JR[3 * i + j];
                Jo[6 * i + 3 + j] = sqrt_info * jrs;
            }
    }
    return c[2] > 0;
}

// DirectLeftSE3::ReprojectionErrorKSE3XYZ / ReprojectionErrorRightCamKSE3XYZ (ceres_parametrization.cpp:107-195, :198-298):
// world point X seen by the left (type 0) or right (type 1, through T_rl) camera of keyframe RTo = (Rwc | t).
// Jp: 2x6 w.r.t. the left-multiplicative pose tangent [-J_R, J_R hat(X)], Jx: 2x3 = J_R.
template <bool JAC>
__device__ __forceinline__ int d_residual_xyz(const BADev &D, int type, const double *RTo, const double *X, const double *uv, double sigma,
                                              double *r, double *Jp, double *Jx)
{
    const double sqrt_info = 1.0 / sigma;
    const double d[3] = {X[0] - RTo[9], X[1] - RTo[10], X[2] - RTo[11]};
    double lc[3], cam[3];
    for (int i = 0; i < 3; i++) lc[i] = RTo[i] * d[0] + RTo[3 + i] * d[1] + RTo[6 + i] * d[2];      // Rcw = Rwc^T
    const double *K = D.calib_l;
    if (type == OV2_XYZ_RIGHT) {
        for (int i = 0; i < 3; i++) cam[i] = D.Rrl[3 * i] * lc[0] + D.Rrl[3 * i + 1] * lc[1] + D.Rrl[3 * i + 2] * lc[2] + D.trl[i];
        K = D.calib_r;
    } else { cam[0] = lc[0]; cam[1] = lc[1]; cam[2] = lc[2]; }
    const double invz = 1.0 / cam[2];
    r[0] = sqrt_info * (K[0] * cam[0] * invz + K[2] - uv[0]);
    r[1] = sqrt_info * (K[1] * cam[1] * invz + K[3] - uv[1]);
    const int dp = cam[2] > 0;
    if (!JAC) return dp;
    const double invz2 = invz * invz;
    const double Jc[6] = {invz * K[0], 0, -cam[0] * invz2 * K[0], 0, invz * K[1], -cam[1] * invz2 * K[1]};
    double M[9];
    if (type == OV2_XYZ_RIGHT) {
        for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++)
            M[3 * i + j] = D.Rrl[3 * i] * RTo[3 * j] + D.Rrl[3 * i + 1] * RTo[3 * j + 1] + D.Rrl[3 * i + 2] * RTo[3 * j + 2];
    } else for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) M[3 * i + j] = RTo[3 * j + i];
    double JR[6];
    for (int i = 0; i < 2; i++) for (int j = 0; j < 3; j++) JR[3 * i + j] = sqrt_info * (Jc[3 * i] * M[j] + Jc[3 * i + 1] * M[3 + j] + Jc[3 * i + 2] * M[6 + j]);
    for (int i = 0; i < 2; i++) {
        const double a = JR[3 * i], b = JR[3 * i + 1], c = JR[3 * i + 2];
        Jx[3 * i] = a; Jx[3 * i + 1] = b; Jx[3 * i + 2] = c;
        Jp[6 * i] = -a; Jp[6 * i + 1] = -b; Jp[6 * i + 2] = -c;
        Jp[6 * i + 3] = b * X[2] - c * X[1];                  // J_R hat(X)
        Jp[6 * i + 4] = c * X[0] - a * X[2];
        Jp[6 * i + 5] = a * X[1] - b * X[0];
    }
    return dp;
}

__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// sum over the workgroup (<= 16 wavefronts); result valid in thread 0
__device__ __forceinline__ double block_sum(double v, double *s_part)
{
    v = wave_sum(v);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, nw = (blockDim.x + 63) >> 6;
    __syncthreads();
    if (lane == 0) s_part[wave] = v;
    __syncthreads();
    double t = 0;
    if (threadIdx.x == 0) for (int w = 0; w < nw; w++) t += s_part[w];
    return t;
}

// three sums (or, MAX = true, maxima) over the workgroup with two barriers; results valid in thread 0.  The
// single-workgroup bookkeeping kernels used 10-step LDS trees per value: ~11 barriers of 16 wavefronts each.
template <bool MAX>
__device__ __forceinline__ void block_reduce3(double &a, double &b, double &c, double (*s_part)[16])
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const double ta = __shfl_xor(a, off, 64), tb = __shfl_xor(b, off, 64), tc = __shfl_xor(c, off, 64);
        if (MAX) { a = fmax(a, ta); b = fmax(b, tb); c = fmax(c, tc); } else { a += ta; b += tb; c += tc; }
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, nw = (blockDim.x + 63) >> 6;
    __syncthreads();
    if (lane == 0) { s_part[0][wave] = a; s_part[1][wave] = b; s_part[2][wave] = c; }
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < nw; w++) {
            if (MAX) { a = fmax(a, s_part[0][w]); b = fmax(b, s_part[1][w]); c = fmax(c, s_part[2][w]); }
            else { a += s_part[0][w]; b += s_part[1][w]; c += s_part[2][w]; }
        }
}

// ---------------------------------------------------------------------------------- linearize
// Persistent wavefronts: wave w owns a contiguous chunk of the anchor-sorted landmark order, one lane
// per residual block.  Pose-side sums are pre-aggregated in LDS (fp64 ds_add):
//   block-shared  Hoo[n_opt][21], bo[n_opt][6]        (observer diagonal blocks, F^T b)
//   per-wave      Hao[n_opt][36]                      (anchor x observer blocks of the CURRENT anchor)
//   per-wave regs Haa[21], ba[6]                      (anchor diagonal block, flushed when the anchor changes)
// and reach HBM as a few thousand atomics per workgroup instead of ~60 per residual block.
// H is stored as its UPPER triangle only (row <= col).
// The 35 per-landmark sums over the residual lanes (Haa[21], F_a^T b [6], E^T F_a [6], E^T E, E^T b) go through a
// per-wave 35 x 33 LDS transpose -- every lane parks its partials, lane q adds up row q -- instead of 35 six-step
// shuffle butterflies (420 ds_bpermute per landmark: a third of this kernel by knock-out timing); lane q keeps
// the running anchor sums q < 27 in ONE register until the anchor changes.
// dynamic LDS: 8*nfp (two W rows per wavefront) + n_opt*27 + 4*n_opt*21 + 4*LIN_RED doubles
#define LIN_NRED 35
#define LIN_RED (LIN_NRED * 33)
__device__ __forceinline__ void h_add_upper(double *H, int ld, int r, int c, double v)
{
    if (r <= c) atomicAdd(&H[(long long)r * ld + c], v); else atomicAdd(&H[(long long)c * ld + r], v);
}

// BIG: the sparse-W variant for reduced systems beyond the LDS-resident limit (BADev::big): nothing is aggregated in LDS but
// the per-wave reduction scratch and the observers' diagonal blocks / F^T b; anchor-observer blocks go to H with global atomics,
// the landmark's W entries to their slots in cww.
template <bool BIG>
__device__ __forceinline__ void b_ba_linearize(const BADev &D, const int *__restrict__ lm_order)
{
    BACtl *ctl = D.ctl;
    if (ctl->done || !ctl->need_lin) return;
    extern __shared__ __align__(16) unsigned char smem_raw[];
    const int n_opt = D.nf / 6, n_hao = BIG ? 0 : n_opt * 21;      // BIG: no per-wavefront anchor-observer cache, no dense W row
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const bool direct = BIG && D.lin_direct;                        // no LDS pre-aggregation of the observer blocks at all
    // (deterministic mode: this work-group is ONE wavefront and owns a copy of H and F^T b -- nothing it adds to races with anything)
    double *Hout = (!BIG && D.det) ? D.Hpart + (size_t)blockIdx.x * D.nfp * D.nfp : D.H;
    double *bfout = (!BIG && D.det) ? D.bfpart + (size_t)blockIdx.x * D.nfp : D.bf;
    const int n_agg = direct ? 0 : n_opt;
    double *wrow = (double *)smem_raw + wave * (BIG ? 0 : 2 * D.nfp);   // two rows: a pair of landmarks (below)
    double *Hoo = (double *)smem_raw + 8 * (BIG ? 0 : D.nfp);
    double *bo = Hoo + n_agg * 21;
    double *Hao = bo + n_agg * 6 + wave * n_hao;
    double *red = bo + n_agg * 6 + 4 * n_hao + wave * LIN_RED;
    for (int e = threadIdx.x; e < n_agg * 27 + 4 * n_hao; e += blockDim.x) Hoo[e] = 0;
    __syncthreads();

    const int wpb = blockDim.x >> 6, total_waves = gridDim.x * wpb, gw = blockIdx.x * wpb + wave;
    const int chunk = (D.n_lm + total_waves - 1) / total_waves;
    const int i0 = gw * chunk, i1 = min(D.n_lm, i0 + chunk);
    double cost = 0;
    int cur_ca = -1;
    double dacc = 0;                                        // lane q < 21: Haa entry q, lane 21..26: (F_a^T b)[q - 21] of the current anchor
    double gmax_w = 0;                                      // lane 34: max |E^T b| over this wavefront's landmarks (k_ba_iter_begin's gradient norm)

    auto flush_anchor = [&](int ca) {
        if (ca < 0 && BIG) return;                                   // (small path: a fixed anchor's blocks still carry the observers' M)
        if (ca >= 0) {
        // anchor diagonal block + F^T b: lanes 0..26 hold one entry each
        if (lane < 21) {
            int c = 0, d = 0, t = lane;
            for (c = 0; c < 6; c++) { if (t < 6 - c) { d = c + t; break; } t -= 6 - c; }
            if (dacc != 0.0) atomicAdd(&Hout[(long long)(ca + c) * D.nfp + ca + d], dacc);
        } else if (lane < 27) {
            if (dacc != 0.0) atomicAdd(&bfout[ca + lane - 21], dacc);
        }
        }
        // (small path, round 4) the per-wavefront cache holds M = sum J_o^T J_o per observer (21 numbers) for the blocks of the current
        // anchor: in the left-multiplicative tangent J_o = -J_a, so the same numbers are the observer's diagonal block (+M) AND the
        // anchor-observer block (J_a^T J_o = -M) -- 21 LDS atomics per residual block instead of 21 + 36
        for (int e = lane; e < n_hao; e += 64) {
            const double v = Hao[e];
            if (v != 0.0) {
                const int ob = e / 21;
                int t = e - ob * 21, c = 0, d = 0;
                for (c = 0; c < 6; c++) { if (t < 6 - c) { d = c + t; break; } t -= 6 - c; }
                atomicAdd(&Hoo[e], v);                                               // block-shared observer blocks (same indexing)
                if (ca >= 0) {
                    h_add_upper(Hout, D.nfp, ca + d, ob * 6 + c, -v);
                    if (d != c) h_add_upper(Hout, D.nfp, ca + c, ob * 6 + d, -v);
                }
                Hao[e] = 0;
            }
        }
        dacc = 0;
    };

    // Two-stage software pipeline over the landmarks of this wavefront (one wavefront per SIMD: nothing else hides the
    // dependent global round trips order -> header -> residual records -> poses): the header of landmark idx+2 and the
    // residual records of the first 64 blocks of landmark idx+1 are requested before landmark idx is processed.
    struct LmHdr { int lm, beg, end, a, ca; double lam, au, av; };
    struct ResRec { int type, kf, orig, off; double u, v, sigma; };
    auto load_hdr = [&](int idx) {
        LmHdr h;
        h.lm = lm_order[min(idx, i1 - 1)];
        h.beg = D.lm_ptr[h.lm]; h.end = D.lm_ptr[h.lm + 1];
        h.a = D.lm_anchor[h.lm]; h.ca = D.pose_col[h.a];
        h.lam = D.x_lam[h.lm]; h.au = D.lm_auv[2 * h.lm]; h.av = D.lm_auv[2 * h.lm + 1];
        return h;
    };
    auto load_rec = [&](const LmHdr &hx, const LmHdr &hy, bool pair) {
        ResRec r;
        const bool hi = pair && lane >= 32;                        // (a pair: landmark y's blocks in the lanes 32 .. 63)
        const int hb = hi ? hy.beg : hx.beg, he = hi ? hy.end : hx.end;
        const int k = max(0, min(hb + (pair ? lane & 31 : lane), he - 1));       // (a landmark without residual blocks: nothing is consumed)
        r.type = D.res_type[k]; r.kf = D.res_kf[k]; r.orig = D.res_orig[k]; r.off = D.res_off ? D.res_off[k] : 0;
        r.u = D.res_uv[2 * k]; r.v = D.res_uv[2 * k + 1]; r.sigma = D.res_sigma[k];
        return r;
    };
    // Round 4: TWO landmarks per wavefront where that is possible -- a landmark of the local-BA window has ~30 residual blocks, a
    // lane per block left half the wavefront idle on every SIMD's only wavefront.  Consecutive landmarks (the order groups them by
    // anchor) with the same anchor keyframe and at most 32 blocks each share a step: landmark x in the lanes 0 .. 31, landmark y in
    // 32 .. 63, one W row each, the same anchor accumulators and anchor-observer cache, and the transpose-reduce's two half-wave
    // passes deliver the two landmarks' sums.  Anything else (more blocks, a change of anchor, the sparse-W path) goes singly.
    LmHdr hq0, hq1, hq2, hq3;                                       // headers of the landmarks idx .. idx + 3
    ResRec r_cur;
    auto pairable = [&](const LmHdr &x, const LmHdr &y, int ix) { return !BIG && ix + 1 < i1 && x.a == y.a && x.end - x.beg <= 32 && y.end - y.beg <= 32; };
    bool pair_cur = false;
    if (i0 < i1) {
        hq0 = load_hdr(i0); hq1 = load_hdr(i0 + 1); hq2 = load_hdr(i0 + 2); hq3 = load_hdr(i0 + 3);
        pair_cur = pairable(hq0, hq1, i0);
        r_cur = load_rec(hq0, hq1, pair_cur);
    }
    for (int idx = i0; idx < i1;) {
        const int nidx = idx + (pair_cur ? 2 : 1);
        const LmHdr n0 = pair_cur ? hq2 : hq1, n1 = pair_cur ? hq3 : hq2;
        const bool pair_nxt = nidx < i1 && pairable(n0, n1, nidx);
        const ResRec r_nxt = load_rec(n0, n1, pair_nxt);
        const LmHdr hn0 = load_hdr(idx + 4), hn1 = load_hdr(idx + 5);
        const bool hiB = pair_cur && lane >= 32;                    // this lane works on the second landmark of the pair
        const int lm0 = hq0.lm, lm1 = hq1.lm;
        const int beg = hiB ? hq1.beg : hq0.beg, end = hiB ? hq1.end : hq0.end;
        const int a = hq0.a;
        const int ca = hq0.ca;
        if (ca != cur_ca) { wave_lds_sync(); flush_anchor(cur_ca); wave_lds_sync(); cur_ca = ca; }
        if (!BIG) for (int c = lane; c < (pair_cur ? 2 : 1) * D.nfp; c += 64) wrow[c] = 0;
        wave_lds_sync();
        double *my_wrow = wrow + (hiB ? D.nfp : 0);
        const double lam = hiB ? hq1.lam : hq0.lam;
        const double auv[2] = {hiB ? hq1.au : hq0.au, hiB ? hq1.av : hq0.av};
        double ete = 0, etb = 0, wa[6] = {0, 0, 0, 0, 0, 0}, ba[6] = {0, 0, 0, 0, 0, 0}, Haa[21];
        for (int k = 0; k < 21; k++) Haa[k] = 0;
        const int nbatch = pair_cur ? 1 : (hq0.end - hq0.beg + 63) / 64;      // (wave-uniform)
        for (int bt = 0; bt < nbatch; bt++) {
            const int k = beg + 64 * bt + (pair_cur ? lane & 31 : lane);
            const bool first = bt == 0;                                       // (wave-uniform) records of the first batch were prefetched
            if (k < end && !(first ? r_cur.off : (D.res_off ? (int)D.res_off[k] : 0))) {   // removed blocks keep their cached chi2 (N4)
                const int type = first ? r_cur.type : D.res_type[k];
                const int o = type == OV2_RES_RIGHT_ANCH ? a : (first ? r_cur.kf : D.res_kf[k]);
                const int co = type == OV2_RES_RIGHT_ANCH ? -1 : D.pose_col[o];
                const int cae = type == OV2_RES_RIGHT_ANCH ? -1 : ca;
                const double uv[2] = {first ? r_cur.u : D.res_uv[2 * k], first ? r_cur.v : D.res_uv[2 * k + 1]};
                double r[2], Ja[12], Jo[12], Jl[2];
                const int dp = d_residual<true>(D, type, D.x_RT + 12 * a, D.x_RT + 12 * o, lam, auv, uv, first ? r_cur.sigma : D.res_sigma[k], r, Ja, Jo, Jl);
                const double s = r[0] * r[0] + r[1] * r[1];
                const int orig = first ? r_cur.orig : D.res_orig[k];
                D.chi2[orig] = s; D.dpos[orig] = (uint8_t)dp;
                double rho0, rho1;
                d_huber(D.huber, s, rho0, rho1);
                cost += 0.5 * rho0;
                // corrector.cc: rho'' <= 0 for Huber / trivial loss -> scale residual and Jacobians by sqrt(rho')
                const double sc = sqrt(rho1);
                r[0] *= sc; r[1] *= sc; Jl[0] *= sc; Jl[1] *= sc;
                for (int q = 0; q < 12; q++) { Ja[q] *= sc; Jo[q] *= sc; }
                ete += Jl[0] * Jl[0] + Jl[1] * Jl[1];
                etb += Jl[0] * r[0] + Jl[1] * r[1];
                if (cae >= 0) {
                    int t = 0;
                    for (int c = 0; c < 6; c++) {
                        wa[c] += Jl[0] * Ja[c] + Jl[1] * Ja[6 + c];
                        ba[c] += Ja[c] * r[0] + Ja[6 + c] * r[1];
                        for (int d = c; d < 6; d++) Haa[t++] += Ja[c] * Ja[d] + Ja[6 + c] * Ja[6 + d];
                    }
                }
                if (BIG) {
                    // sparse W: this block's observer entry joins its (landmark, keyframe) slot; the observer's diagonal block and
                    // F^T b are aggregated in LDS as in the small path, only the anchor-observer block goes straight to HBM
                    if (co >= 0) {
                        const int ob = co / 6;
                        double *slot = D.cww + (long long)6 * D.res_cw[k];
                        int t = 0;
                        for (int c = 0; c < 6; c++) {
                            atomicAdd(&slot[c], Jl[0] * Jo[c] + Jl[1] * Jo[6 + c]);
                            if (direct) {
                                atomicAdd(&D.bf[co + c], Jo[c] * r[0] + Jo[6 + c] * r[1]);
                                for (int d = c; d < 6; d++) atomicAdd(&D.H[(long long)(co + c) * D.nfp + co + d], Jo[c] * Jo[d] + Jo[6 + c] * Jo[6 + d]);
                            } else {
                            atomicAdd(&bo[ob * 6 + c], Jo[c] * r[0] + Jo[6 + c] * r[1]);
                            for (int d = c; d < 6; d++) atomicAdd(&Hoo[ob * 21 + t++], Jo[c] * Jo[d] + Jo[6 + c] * Jo[6 + d]);
                            }
                            if (cae >= 0)
                                for (int d = 0; d < 6; d++) h_add_upper(D.H, D.nfp, cae + d, co + c, Ja[d] * Jo[c] + Ja[6 + d] * Jo[6 + c]);
                        }
                    }
                } else
                if (co >= 0) {
                    const int ob = co / 6;
                    int t = 0;
                    for (int c = 0; c < 6; c++) {
                        atomicAdd(&my_wrow[co + c], Jl[0] * Jo[c] + Jl[1] * Jo[6 + c]);   // LDS fp64 atomics
                        atomicAdd(&bo[ob * 6 + c], Jo[c] * r[0] + Jo[6 + c] * r[1]);
                        for (int d = c; d < 6; d++) atomicAdd(&Hao[ob * 21 + t++], Jo[c] * Jo[d] + Jo[6 + c] * Jo[6 + d]);
                    }
                }
            }
        }
        // transpose-reduce: slots 0..20 Haa, 21..26 ba, 27..32 wa, 33 E^T E, 34 E^T b; pass p takes the lanes 32 p .. 32 p + 31: the
        // second landmark of a pair, or the blocks 32 .. 63 of a single landmark with more than 32 of them
        double tot = 0, totB = 0;
        for (int p = 0; p < ((pair_cur || hq0.end - hq0.beg > 32) ? 2 : 1); p++) {
            if ((lane >> 5) == p) {
                double *col = red + (lane & 31);
#pragma unroll
                for (int k = 0; k < 21; k++) col[k * 33] = Haa[k];
#pragma unroll
                for (int c = 0; c < 6; c++) { col[(21 + c) * 33] = ba[c]; col[(27 + c) * 33] = wa[c]; }
                col[33 * 33] = ete; col[34 * 33] = etb;
            }
            wave_lds_sync();
            if (lane < LIN_NRED) {
                const double *row = red + lane * 33;
                double t = 0;
#pragma unroll
                for (int j = 0; j < 32; j++) t += row[j];
                if (pair_cur && p == 1) totB += t; else tot += t;
            }
            wave_lds_sync();
        }
        if (ca >= 0 && lane < 27) dacc += tot + totB;
        if (lane == 33) { D.ete[lm0] = tot; if (pair_cur) D.ete[lm1] = totB; }
        if (lane == 34) { D.etb[lm0] = tot; if (pair_cur) D.etb[lm1] = totB; gmax_w = fmax(gmax_w, fmax(fabs(tot), fabs(totB))); }
        if (BIG) {
            const int sa = D.lm_cwa[lm0];                                                            // the landmark's anchor entry of W
            if (sa >= 0 && lane >= 27 && lane < 33) atomicAdd(&D.cww[(long long)6 * sa + lane - 27], tot);
        } else {
            if (ca >= 0 && lane >= 27 && lane < 33) { wrow[ca + lane - 27] += tot; if (pair_cur) wrow[D.nfp + ca + lane - 27] += totB; }
            wave_lds_sync();
            double *Wg = D.W + (long long)lm0 * D.nfp;
            for (int c = lane; c < D.nfp; c += 64) Wg[c] = wrow[c];
            if (pair_cur) {
                double *Wh = D.W + (long long)lm1 * D.nfp;
                for (int c = lane; c < D.nfp; c += 64) Wh[c] = wrow[D.nfp + c];
            }
        }
        wave_lds_sync();
        if (pair_cur) { hq0 = hq2; hq1 = hq3; hq2 = hn0; hq3 = hn1; }
        else { hq0 = hq1; hq1 = hq2; hq2 = hq3; hq3 = hn0; }
        idx = nidx; pair_cur = pair_nxt; r_cur = r_nxt;
    }
    wave_lds_sync();
    flush_anchor(cur_ca);
    __syncthreads();
    // block-shared observer blocks
    for (int e = threadIdx.x; e < n_agg * 21; e += blockDim.x) {
        const double v = Hoo[e];
        if (v != 0.0) {
            const int ob = e / 21;
            int t = e - ob * 21, c = 0, d = 0;
            for (c = 0; c < 6; c++) { if (t < 6 - c) { d = c + t; break; } t -= 6 - c; }
            atomicAdd(&Hout[(long long)(ob * 6 + c) * D.nfp + ob * 6 + d], v);
        }
    }
    for (int e = threadIdx.x; e < n_agg * 6; e += blockDim.x) { const double v = bo[e]; if (v != 0.0) atomicAdd(&bfout[e], v); }
    __shared__ double s_part[4];
    cost = block_sum(cost, s_part);
    if (threadIdx.x == 0) { if (!BIG && D.det) D.costpart[blockIdx.x] = cost; else if (cost != 0.0) atomicAdd(&ctl->cost_acc, cost); }
    // max |E^T b| of this work-group's landmarks: slot blockIdx.x of row 6 of BADev::part (k_ba_iter_begin takes the maximum of
    // the slots instead of walking the landmarks with one work-group)
    __shared__ double s_gm[4];
    if (lane == 34) s_gm[wave] = gmax_w;
    __syncthreads();
    if (threadIdx.x == 0 && D.part) { double g = 0; for (int w = 0; w < wpb; w++) g = fmax(g, s_gm[w]); D.part[6 * BA_PART_MAX + blockIdx.x] = g; }
}
template <bool BIG>
__global__ __launch_bounds__(256) void k_ba_linearize(BADev D, const int *__restrict__ lm_order) { b_ba_linearize<BIG>(D, lm_order); }
__global__ __launch_bounds__(256) void k_ba_linearize_B(const BADev *__restrict__ arr) { const BADev &D = arr[blockIdx.z]; b_ba_linearize<false>(D, D.lm_order_b); }

// ---------------------------------------------------------------------------------- pose-only residual blocks
// rows without an e-block (Ceres: SchurEliminator::NoEBlockRowsUpdate): F^T F / F^T b pre-aggregated per workgroup in LDS.
// dynamic LDS: n_opt * 27 doubles
__global__ __launch_bounds__(256) void k_ba_linearize_po(BADev D)
{
    BACtl *ctl = D.ctl;
    if (ctl->done || !ctl->need_lin) return;
    extern __shared__ __align__(16) unsigned char smem_raw[];
    const bool direct = D.big && D.lin_direct;
    const int n_opt = direct ? 0 : D.nf / 6;                          // (direct: nothing is pre-aggregated in LDS)
    double *Hoo = (double *)smem_raw, *bo = Hoo + n_opt * 21;
    // (deterministic mode: one wavefront per work-group, its own copy of H / F^T b -- after the landmark lineariser's copies)
    double *Hout = D.det ? D.Hpart + (size_t)(D.det_lin + blockIdx.x) * D.nfp * D.nfp : D.H;
    double *bfout = D.det ? D.bfpart + (size_t)(D.det_lin + blockIdx.x) * D.nfp : D.bf;
    for (int e = threadIdx.x; e < n_opt * 27; e += blockDim.x) Hoo[e] = 0;
    __syncthreads();
    double cost = 0;
    for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < D.n_po; k += gridDim.x * blockDim.x) {
        const int o = D.po_kf[k], co = D.pose_col[o];
        double r[2], Jo[12];
        const int dp = d_residual_pnp<true>(D, D.x_RT + 12 * o, D.po_xyz + 3 * k, D.po_uv + 2 * k, D.po_sigma[k], r, Jo);
        const double s = r[0] * r[0] + r[1] * r[1];
        const int orig = D.po_orig[k];
        D.chi2[orig] = s; D.dpos[orig] = (uint8_t)dp;
        double rho0, rho1;
        d_huber(D.huber, s, rho0, rho1);
        cost += 0.5 * rho0;
        if (co < 0) continue;
        const double sc = sqrt(rho1);
        r[0] *= sc; r[1] *= sc;
        for (int q = 0; q < 12; q++) Jo[q] *= sc;
        const int ob = co / 6;
        int t = 0;
        for (int c = 0; c < 6; c++) {
            if (direct) {
                atomicAdd(&D.bf[co + c], Jo[c] * r[0] + Jo[6 + c] * r[1]);
                for (int d = c; d < 6; d++) atomicAdd(&D.H[(long long)(co + c) * D.nfp + co + d], Jo[c] * Jo[d] + Jo[6 + c] * Jo[6 + d]);
                continue;
            }
            atomicAdd(&bo[ob * 6 + c], Jo[c] * r[0] + Jo[6 + c] * r[1]);
            for (int d = c; d < 6; d++) atomicAdd(&Hoo[ob * 21 + t++], Jo[c] * Jo[d] + Jo[6 + c] * Jo[6 + d]);
        }
    }
    __syncthreads();
    for (int e = threadIdx.x; e < n_opt * 21; e += blockDim.x) {
        const double v = Hoo[e];
        if (v != 0.0) {
            const int ob = e / 21;
            int t = e - ob * 21, c = 0, d = 0;
            for (c = 0; c < 6; c++) { if (t < 6 - c) { d = c + t; break; } t -= 6 - c; }
            atomicAdd(&Hout[(long long)(ob * 6 + c) * D.nfp + ob * 6 + d], v);
        }
    }
    for (int e = threadIdx.x; e < n_opt * 6; e += blockDim.x) { const double v = bo[e]; if (v != 0.0) atomicAdd(&bfout[e], v); }
    __shared__ double s_part[4];
    cost = block_sum(cost, s_part);
    if (threadIdx.x == 0) { if (D.det) D.costpart[D.det_lin + blockIdx.x] = cost; else if (cost != 0.0) atomicAdd(&ctl->cost_acc, cost); }
}

// ---------------------------------------------------------------------------------- cost only
__device__ __forceinline__ void b_ba_cost(const BADev &D)
{
    BACtl *ctl = D.ctl;
    if (ctl->done || !ctl->step_valid) return;
    // half a wavefront per landmark (round 4): a landmark of the local-BA window has ~30 residual blocks -- a wavefront per
    // landmark left half of its lanes idle
    const int l32 = threadIdx.x & 31;
    double cost = 0;
    for (int lm = blockIdx.x * 8 + (threadIdx.x >> 5); lm < D.n_lm; lm += gridDim.x * 8) {
        const int beg = D.lm_ptr[lm], end = D.lm_ptr[lm + 1];
        const int a = D.lm_anchor[lm];
        const double lam = D.c_lam[lm];
        const double auv[2] = {D.lm_auv[2 * lm], D.lm_auv[2 * lm + 1]};
        for (int k = beg + l32; k < end; k += 32) {
            if (D.res_off && D.res_off[k]) continue;
            const int type = D.res_type[k];
            const int o = type == OV2_RES_RIGHT_ANCH ? a : D.res_kf[k];
            const double uv[2] = {D.res_uv[2 * k], D.res_uv[2 * k + 1]};
            double r[2];
            const int dp = d_residual<false>(D, type, D.c_RT + 12 * a, D.c_RT + 12 * o, lam, auv, uv, D.res_sigma[k], r, nullptr, nullptr, nullptr);
            const double s = r[0] * r[0] + r[1] * r[1];
            const int orig = D.res_orig[k];
            D.chi2[orig] = s; D.dpos[orig] = (uint8_t)dp;
            double rho0, rho1;
            d_huber(D.huber, s, rho0, rho1);
            cost += 0.5 * rho0;
        }
    }
    for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < D.n_po; k += gridDim.x * blockDim.x) {
        double r[2];
        const int o = D.po_kf[k];
        const int dp = d_residual_pnp<false>(D, D.c_RT + 12 * o, D.po_xyz + 3 * k, D.po_uv + 2 * k, D.po_sigma[k], r, nullptr);
        const double s = r[0] * r[0] + r[1] * r[1];
        const int orig = D.po_orig[k];
        D.chi2[orig] = s; D.dpos[orig] = (uint8_t)dp;
        double rho0, rho1;
        d_huber(D.huber, s, rho0, rho1);
        cost += 0.5 * rho0;
    }
    __shared__ double s_part[4];
    cost = block_sum(cost, s_part);
    if (threadIdx.x == 0) D.part[5 * BA_PART_MAX + blockIdx.x] = cost;      // summed by k_ba_decide
}
__global__ __launch_bounds__(256) void k_ba_cost(BADev D) { b_ba_cost(D); }
__global__ __launch_bounds__(256) void k_ba_cost_B(const BADev *__restrict__ arr) { const BADev &D = arr[blockIdx.z]; b_ba_cost(D); }

// ---------------------------------------------------------------------------------- deterministic mode: the linearisers' copies, in order
// H = sum of the det_lin + det_po copies (upper-triangle tiles), F^T b likewise, the cost; the copies are cleared for the next
// linearisation as they are read.  Runs right after the linearisers, under the same condition.
__global__ __launch_bounds__(256) void k_ba_det_reduce(BADev D)
{
    BACtl *ctl = D.ctl;
    if (ctl->done || !ctl->need_lin) return;
    const int ncopy = D.det_lin + D.det_po;
    const long long nn = (long long)D.nfp * D.nfp, stride = (long long)gridDim.x * blockDim.x;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < nn; e += stride) {
        const int r = (int)(e / D.nfp), c = (int)(e - (long long)r * D.nfp);
        if (c < (r & ~31)) continue;                            // (left of the diagonal tile: never written)
        // (loads first, in batches of eight, then the stores: a load-add-store per copy made every copy a dependent round trip)
        const double *__restrict__ src = D.Hpart + e;
        double t = 0;
        int q = 0;
        for (; q + 8 <= ncopy; q += 8) {
            double v[8];
#pragma unroll
            for (int u = 0; u < 8; u++) v[u] = src[(size_t)(q + u) * nn];
#pragma unroll
            for (int u = 0; u < 8; u++) t += v[u];
        }
        for (; q < ncopy; q++) t += src[(size_t)q * nn];
        for (q = 0; q < ncopy; q++) D.Hpart[(size_t)q * nn + e] = 0;
        D.H[e] = t;
    }
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < D.nfp; e += stride) {
        double t = 0;
        for (int q = 0; q < ncopy; q++) { double *src = D.bfpart + (size_t)q * D.nfp + e; t += *src; *src = 0; }
        D.bf[e] = t;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        double t = 0;
        for (int q = 0; q < ncopy; q++) { t += D.costpart[q]; D.costpart[q] = 0; }
        ctl->cost_acc += t;
    }
}

// ---------------------------------------------------------------------------------- iteration begin (1 block)
__device__ __forceinline__ void b_ba_iter_begin(const BADev &D, BAOpt O, int seq)
{
    BACtl *ctl = D.ctl;
    (void)seq;
    if (ctl->done) return;
    __shared__ double s_part[3][16];
    __shared__ double s_gmax;
    const int tid = threadIdx.x, nt = blockDim.x;
    // (the linearisers that ran since the last call -- they run when need_lin is set -- produced a linearisation: what the
    // one-thread kernel k_ba_lin_done used to record between them and this kernel)
    const int fresh = ctl->fresh_lin | ctl->need_lin;
    if (fresh) {
        // a new linearisation at x is available: jacobi scaling (iteration 0 only), gradient max-norm
        if (O.jacobi && !ctl->scaled) {
            for (int c = tid; c < D.nf; c += nt) D.scale_f[c] = 1.0 / (1.0 + sqrt(D.H[(long long)c * D.nfp + c]));
            if (D.ldim == 1) for (int l = tid; l < D.n_lm; l += nt) D.scale_l[l] = 1.0 / (1.0 + sqrt(D.ete[l]));
            else for (int l = tid; l < 3 * D.n_lm; l += nt) { const int k = l % 3; D.scale_l[l] = 1.0 / (1.0 + sqrt(D.ete6[6 * (l / 3) + (k == 0 ? 0 : (k == 1 ? 3 : 5))])); }
        }
        // |x - Plus(x, -g)|_inf  (trust_region_minimizer.cc:283-297)
        double gm = 0;
        for (int k = tid; k < D.n_kf; k += nt) {
            const int pc = D.pose_col[k];
            if (pc < 0) continue;
            double d[6], out[7];
            for (int c = 0; c < 6; c++) d[c] = -D.bf[pc + c];
            d_se3_left_plus(D.x_pose + 7 * k, d, out);
            for (int c = 0; c < 7; c++) gm = fmax(gm, fabs(D.x_pose[7 * k + c] - out[c]));
        }
        if (D.ldim == 1) {
            // (per-work-group maxima of the lineariser; landmarks without live blocks have E^T b = 0 there)
            if (D.n_lm > 0) for (int i = tid; i < D.lin_blocks; i += nt) gm = fmax(gm, D.part[6 * BA_PART_MAX + i]);
        } else {
            for (int l = tid; l < 3 * D.n_lm; l += nt)
                if (D.lm_ptr[l / 3] != D.lm_ptr[l / 3 + 1]) gm = fmax(gm, fabs(D.etb[l]));      // Plus(x, -g) - x = -g for a Euclidean block
        }
        double z0 = 0, z1 = 0;
        block_reduce3<true>(gm, z0, z1, s_part);
        if (tid == 0) s_gmax = gm;
    }
    __syncthreads();
    if (tid == 0) {
        // the control block is worked on in registers: one load batch, one store batch (every ctl-> access used to be a
        // dependent global round trip of thread 0)
        BACtl cl = *ctl;
        cl.need_lin = 0; cl.fresh_lin = fresh;
        d_ctl_iter_begin(cl, O, fresh, s_gmax);
        *D.ctl = cl;
    }
    __syncthreads();
    if (ctl->done) return;
    // LevenbergMarquardtStrategy::ComputeStep: diagonal of the (scaled) J^T J, clamped, unless reused
    const double radius = ctl->radius;
    const int reuse = ctl->reuse_diag;
    if (tid == 0) ctl->reuse_now = reuse;
    for (int c = tid; c < D.nfp; c += nt) {
        if (c < D.nf) {
            if (!reuse) {
                const double s = D.scale_f[c];
                D.diag_f[c] = fmin(fmax(s * s * D.H[(long long)c * D.nfp + c], O.min_diag), O.max_diag);
            }
        }
        D.v[c] = 0;
    }
    if (D.ldim == 3) {
        // 3-D point landmarks: only the clamped LM diagonal is formed here; the 3x3 inverses, the rows of Wp and L_c^T E^T b are the
        // work of k_ba_xyz_prep (many work-groups) right after this kernel
        if (!reuse)
            for (int l = tid; l < 3 * D.n_lm; l += nt) {
                const int k = l % 3;
                const double s = D.scale_l[l];
                D.diag_l[l] = fmin(fmax(s * s * D.ete6[6 * (l / 3) + (k == 0 ? 0 : (k == 1 ? 3 : 5))], O.min_diag), O.max_diag);
            }
    } else if (D.big) {
        // (large path: k_ba_schur_sparse reads c_l; the small path's consumers form it themselves, d_lm_c)
        // one workgroup walks all landmarks: the loads of four iterations are issued together (restrict-qualified views:
        // without them every store fences the next iteration's loads -- ten dependent L2 round trips per thread)
        const int *__restrict__ lm_ptr = D.lm_ptr;
        const double *__restrict__ scale_l = D.scale_l, *__restrict__ ete = D.ete, *__restrict__ etb = D.etb;
        double *__restrict__ diag_l = D.diag_l, *__restrict__ cl = D.cl, *__restrict__ ce = D.ce;
#pragma unroll 4
        for (int l = tid; l < D.n_lm; l += nt) {
            const bool has = D.lm_live ? D.lm_live[l] != 0 : lm_ptr[l] != lm_ptr[l + 1];
            const double s = scale_l[l], e = ete[l], b = etb[l];
            const double dg = reuse ? diag_l[l] : fmin(fmax(s * s * e, O.min_diag), O.max_diag);
            const double etep = s * s * e + dg / radius;                  // scaled E^T E + D_e^2
            const double c = has ? s * s / etep : 0.0;
            if (has && !reuse) diag_l[l] = dg;
            cl[l] = c; ce[l] = has ? c * b : 0.0;
        }
    }
    __syncthreads();
    if (tid == 0) ctl->reuse_diag = 1;
}
__global__ __launch_bounds__(1024) void k_ba_iter_begin(BADev D, BAOpt O, int seq) { b_ba_iter_begin(D, O, seq); }
__global__ __launch_bounds__(1024) void k_ba_iter_begin_B(const BADev *__restrict__ arr, BAOpt O, int seq) { const BADev &D = arr[blockIdx.z]; b_ba_iter_begin(D, O, seq); }

// ---------------------------------------------------------------------------------- W^T C W (+ W^T (c etb))
// grid: (n_upper_tiles, ksplit); block 256 threads, each thread a 2x2 patch of a 32x32 tile
__device__ __forceinline__ void b_ba_schur_gemm(const BADev &D, int ntiles, int lm_per_split)
{
    if (D.ctl->done) return;
    // decode upper-triangular tile index
    int t = blockIdx.x, ti = 0;
    while (t >= ntiles - ti) { t -= ntiles - ti; ti++; }
    const int tj = ti + t;
    __shared__ double As[BA_TILE][BA_TILE + 1], Bs[BA_TILE][BA_TILE + 1];
    __shared__ double ces[BA_TILE], cs[BA_TILE];
    const int tid = threadIdx.x;
    // c_l of the step's 32 landmarks by the threads 0..31 (d_lm_c; the 3-D point form comes with C folded into Wp: c = 1)
    const double radius = D.ctl->radius;
    const int reuse = D.ctl->reuse_now;
    const int l0 = blockIdx.y * lm_per_split;
    const int l1 = min(D.n_lm, l0 + lm_per_split);
    // each of the 4 wavefronts owns a 16x16 quadrant of the tile on the fp64 matrix cores: per 4 landmarks one
    // v_mfma_f64_16x16x4_f64 fed by two LDS reads per lane (the VALU version read 4 doubles per 4 FMAs: LDS-bound).
    // Operands: A[i][k] = As[k][i] (lane: i = lane & 15, k = lane >> 4), B[k][j] = Bs[k][j]; D: col = lane & 15,
    // row = (lane >> 4) + 4 reg.
    typedef double d4 __attribute__((ext_vector_type(4)));
    const int wv = tid >> 6, lane = tid & 63, qi = wv >> 1, qj = wv & 1, lr = lane & 15, lk = lane >> 4;
    d4 acc = {0., 0., 0., 0.};
    double vacc = 0;                                        // threads 0..31 of diagonal tiles accumulate v
    // 32 landmarks x 32 columns of both panels per step (A pre-multiplied by c_l); the loads of step s+1 are in flight
    // while step s is multiplied
    double ra[4], rb[4], rc = 0, rcl = 0;
    auto fetch = [&](int lb) {
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int e = tid + 256 * u, kk = e >> 5, cc = e & 31;
            const int l = lb + kk;
            double a = 0, b = 0;
            if (l < l1) {
                const double *wr = D.W + (long long)l * D.nfp;
                a = wr[ti * BA_TILE + cc];
                b = wr[tj * BA_TILE + cc];
            }
            ra[u] = a; rb[u] = b;
        }
        rc = (tid < BA_TILE && lb + tid < l1) ? D.etb[lb + tid] : 0.0;
        rcl = (tid < BA_TILE && lb + tid < l1) ? (D.ldim == 3 ? 1.0 : d_lm_c(D, lb + tid, radius, reuse)) : 0.0;
    };
    fetch(l0);
    for (int lb = l0; lb < l1; lb += BA_TILE) {
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int e = tid + 256 * u;
            As[e >> 5][e & 31] = ra[u]; Bs[e >> 5][e & 31] = rb[u];
        }
        if (tid < BA_TILE) { ces[tid] = rc; cs[tid] = rcl; }
        __syncthreads();
        if (lb + BA_TILE < l1) fetch(lb + BA_TILE);
#pragma unroll
        for (int g = 0; g < BA_TILE / 4; g++)
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(As[4 * g + lk][16 * qi + lr] * cs[4 * g + lk], Bs[4 * g + lk][16 * qj + lr], acc, 0, 0, 0);
        if (ti == tj && tid < BA_TILE)
            for (int kk = 0; kk < BA_TILE; kk++) vacc += As[kk][tid] * cs[kk] * ces[kk];
        __syncthreads();
    }
    if (D.det) {
        // deterministic mode: this (tile, landmark split) is the only writer of its entries in the split's copy; k_ba_assemble adds the
        // copies up in order
        double *Gp = D.Gpart + (size_t)blockIdx.y * D.nfp * D.nfp, *vp = D.vpart + (size_t)blockIdx.y * D.nfp;
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int gi = ti * BA_TILE + 16 * qi + lk + 4 * r, gj = tj * BA_TILE + 16 * qj + lr;
            Gp[(long long)gi * D.nfp + gj] = acc[r];
        }
        if (ti == tj && tid < BA_TILE) vp[ti * BA_TILE + tid] = vacc;
        return;
    }
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int gi = ti * BA_TILE + 16 * qi + lk + 4 * r, gj = tj * BA_TILE + 16 * qj + lr;
        if (acc[r] != 0.0) atomicAdd(&D.G[(long long)gi * D.nfp + gj], acc[r]);
    }
    if (ti == tj && tid < BA_TILE && vacc != 0.0) atomicAdd(&D.v[ti * BA_TILE + tid], vacc);
}
__global__ __launch_bounds__(256) void k_ba_schur_gemm(BADev D, int ntiles, int lm_per_split) { b_ba_schur_gemm(D, ntiles, lm_per_split); }
__global__ __launch_bounds__(256) void k_ba_schur_gemm_B(const BADev *__restrict__ arr) { const BADev &D = arr[blockIdx.z]; if ((int)blockIdx.x >= D.g_nupper || (int)blockIdx.y >= D.g_ksplit) return; b_ba_schur_gemm(D, D.g_ntiles, D.g_lmps); }

// ---------------------------------------------------------------------------------- reduced system (1 block)
// S = s_i s_j (H_ij - G_ij) + delta_ij diag_i / radius ; rhs = s_i (b_i - v_i); blocked Cholesky; solve.
// Right-looking, 32-wide panels: the diagonal block is factored in LDS by one wavefront, the panel
// below it is solved row-per-thread against that block and parked in LDS, and the trailing update
// reads the panel from LDS only (each S entry is touched once per panel).
#define CH_NB 32
#define CH_GRP 8           // columns of the diagonal block published per work-group barrier (pipelined panel solve): 2 / 4 / 8 -> 102 / 89 / 87 us
#define CH_LDP 33          // padded leading dimension (doubles) of the LDS panel rows
// knock-out timings of k_ba_cholesky's phases (no MFMA, no loads of the old tile values, no tile stores, no LDS operand reads, a
// quarter of the panel solve's terms): profiles/archive/r4_ba_dead_ends.txt
#define CH_MAX_LDS_N 415   // k_ba_cholesky (512 threads, six panel wavefronts): the right-hand side rides as a panel row, n - 32 + 1 <= 384; larger: HBM path
// dynamic LDS of k_ba_cholesky: diagonal block, solution vector, panel (rows rounded up to whole 16-row MFMA tiles: the trailing
// update reads its operand rows unpredicated)
static inline size_t chol_lds_bytes(int nf, int nfp) { return 8 * ((size_t)CH_NB * CH_LDP + 2 * (size_t)nfp + (size_t)((std::max(0, nf - CH_NB) + 15) & ~15) * CH_LDP) + 64; }

// The two triangular solves L y = rhs, L^T x = y on the factor in S (HBM) with the inverse diagonal blocks in Linv; yv (LDS, nfp
// doubles) holds rhs on entry and x on return, L11 is a CH_NB x CH_LDP LDS scratch.  One work-group.
__device__ __forceinline__ void chol_trisolve(const BADev &D, double *L11, double *yv, double (*s_red)[33], bool forward_done = false)
{
    const int n = D.nf, ld = D.nfp, tid = threadIdx.x, nt = blockDim.x;
    const double *S = D.S, *Linv = D.Linv;
    // forward substitution  L y = rhs, left-looking by blocks:  y_blk = Linv_blk (b_blk - L[blk, 0:k0] y[0:k0])
    // (forward_done: yv already holds y -- k_ba_cholesky carries the right-hand side through the factorisation as one more panel row)
    const int tr = tid >> 5, tcn = tid & 31, ngr = nt >> 5;  // ngr groups of 32 partial-sum threads
    for (int k0 = 0; k0 < n && !forward_done; k0 += CH_NB) {
        const int nb = min(CH_NB, n - k0);
        for (int r = tr; r < CH_NB; r += ngr) {
            double part = 0;
            if (r < nb) for (int k = tcn; k < k0; k += 32) part += S[(long long)(k0 + r) * ld + k] * yv[k];
            s_red[r][tcn] = part;
        }
        for (int e = tid; e < CH_NB * CH_NB; e += nt) L11[(e >> 5) * CH_LDP + (e & 31)] = Linv[(long long)(k0 / CH_NB) * CH_NB * CH_NB + e];
        __syncthreads();
        if (tid < CH_NB) {
            double r = 0;
            for (int q = 0; q < 32; q++) r += s_red[tid][q];
            s_red[tid][32] = tid < nb ? yv[k0 + tid] - r : 0.0;
        }
        __syncthreads();
        if (tid < nb) {
            double r = 0;
            for (int k = 0; k <= tid; k++) r += L11[tid * CH_LDP + k] * s_red[k][32];
            yv[k0 + tid] = r;
        }
        __syncthreads();
    }
    // backward substitution  L^T x = y, right-looking by blocks, last block first:  x_blk = Linv_blk^T y_blk, then
    // y[0:k0] -= L[blk, 0:k0]^T x_blk.  Nothing the loop loads depends on x: thread t keeps column t of the block row L[blk, 0:k0]
    // (32 doubles, coalesced over t) and its share of Linv_blk in registers, requested one block ahead, so that a block costs two
    // barriers and 2 x 32 FMAs instead of a dependent walk over L in L2 with three barriers (round 4: 44 -> ~12 us at n = 300).
    if (n <= nt && nt >= 256) {
        const int nblk = (n + CH_NB - 1) / CH_NB;
        constexpr int NINV = CH_NB * CH_NB / 256;                // Linv doubles per thread at the smallest work-group (256)
        double cur[CH_NB], nxt[CH_NB], winv[NINV], ninv[NINV];
        auto load_rows = [&](int k0, int nb, double (&v)[CH_NB]) {
#pragma unroll
            for (int i = 0; i < CH_NB; i++) v[i] = (tid < k0 && i < nb) ? S[(long long)(k0 + i) * ld + tid] : 0.0;
        };
        auto load_inv = [&](int blk, double (&w)[NINV]) {
#pragma unroll
            for (int u = 0; u < NINV; u++) { const int e = tid + u * nt; w[u] = e < CH_NB * CH_NB ? Linv[(long long)blk * CH_NB * CH_NB + e] : 0.0; }
        };
        load_rows((nblk - 1) * CH_NB, n - (nblk - 1) * CH_NB, cur);
        load_inv(nblk - 1, winv);
        for (int blk = nblk - 1; blk >= 0; blk--) {
            const int k0 = blk * CH_NB, nb = min(CH_NB, n - k0);
#pragma unroll
            for (int u = 0; u < NINV; u++) { const int e = tid + u * nt; if (e < CH_NB * CH_NB) L11[(e >> 5) * CH_LDP + (e & 31)] = winv[u]; }
            if (blk > 0) { load_rows(k0 - CH_NB, CH_NB, nxt); load_inv(blk - 1, ninv); }
            __syncthreads();                                     // the inverse block is staged, y carries every later block's update
            if (tid < CH_NB) {
                double r = 0;
                for (int k = tid; k < nb; k++) r += L11[k * CH_LDP + tid] * yv[k0 + k];     // Linv^T
                s_red[tid][32] = tid < nb ? r : 0.0;
            }
            __syncthreads();
            if (tid < nb) yv[k0 + tid] = s_red[tid][32];
            if (tid < k0) {
                double acc = yv[tid];
#pragma unroll
                for (int i = 0; i < CH_NB; i++) acc -= cur[i] * s_red[i][32];
                yv[tid] = acc;
            }
#pragma unroll
            for (int i = 0; i < CH_NB; i++) cur[i] = nxt[i];
#pragma unroll
            for (int u = 0; u < NINV; u++) winv[u] = ninv[u];
        }
        __syncthreads();
        return;
    }
    // (systems wider than the work-group: the large-problem path) left-looking, x_blk = Linv_blk^T (y_blk - L[below, blk]^T x[below])
    for (int k0 = ((n - 1) / CH_NB) * CH_NB; k0 >= 0; k0 -= CH_NB) {
        const int nb = min(CH_NB, n - k0);
        // lanes along the block's columns (coalesced), thread groups along the rows below
        for (int g = tr; g < 32; g += ngr) {
            double part = 0;
            if (tcn < nb) for (int i = k0 + nb + g; i < n; i += 32) part += S[(long long)i * ld + k0 + tcn] * yv[i];
            s_red[tcn][g] = part;
        }
        for (int e = tid; e < CH_NB * CH_NB; e += nt) L11[(e >> 5) * CH_LDP + (e & 31)] = Linv[(long long)(k0 / CH_NB) * CH_NB * CH_NB + e];
        __syncthreads();
        if (tid < CH_NB) {
            double r = 0;
            for (int q = 0; q < 32; q++) r += s_red[tid][q];
            s_red[tid][32] = tid < nb ? yv[k0 + tid] - r : 0.0;
        }
        __syncthreads();
        if (tid < nb) {
            double r = 0;
            for (int k = tid; k < nb; k++) r += L11[k * CH_LDP + tid] * s_red[k][32];     // Linv^T
            yv[k0 + tid] = r;
        }
        __syncthreads();
    }
}

// Backward substitution  L^T x = y  on the factor in S WITHOUT inverse diagonal blocks (k_ba_cholesky, round 4): right-looking by
// blocks, last block first.  Wavefront 0 solves the block itself -- lane j keeps column j of the 32 x 32 diagonal block in registers
// and the 32 unknowns go by, last first: x_i = y_i / L_ii in lane i, broadcast by v_readlane, y_j -= L_ij x_i in the lanes j < i --;
// the other wavefronts then take the block's unknowns out of everything above: thread t keeps column t of the block row L[blk, 0:k0]
// in registers.  Nothing that is loaded depends on x: both register sets are requested one block ahead.  yv holds y on entry and x on
// return; rd_all = 1 / L_ii of all n unknowns (kept from the factorisation); needs n - 32 <= blockDim - 64.
__device__ __forceinline__ void chol_backward_blocks(const BADev &D, double *yv, const double *rd_all, double *s_x)
{
    const int n = D.nf, ld = D.nfp, tid = threadIdx.x, lane = tid & 63, t = tid - 64;
    const bool w0 = tid < 64;
    const double *S = D.S;
    const int nblk = (n + CH_NB - 1) / CH_NB;
    double cur[CH_NB], nxt[CH_NB], nx2[CH_NB];                   // two blocks ahead: a block's own work is ~1 us, its 32 loads per thread ~3 us
    auto load = [&](int k0, int nb, double (&v)[CH_NB]) {
        const double *col = S + (long long)k0 * ld + (w0 ? k0 + lane : t);
        const bool mine = w0 ? lane < nb : t < k0;
#pragma unroll
        for (int i = 0; i < CH_NB; i++) v[i] = (mine && i < nb && (!w0 || i > lane)) ? col[(long long)i * ld] : 0.0;   // w0: L[i][lane] of the diagonal block; else L[k0 + i][t]
    };
    load((nblk - 1) * CH_NB, n - (nblk - 1) * CH_NB, cur);
#pragma unroll
    for (int i = 0; i < CH_NB; i++) nxt[i] = 0.0;
    if (nblk > 1) load((nblk - 2) * CH_NB, CH_NB, nxt);
    for (int blk = nblk - 1; blk >= 0; blk--) {
        const int k0 = blk * CH_NB, nb = min(CH_NB, n - k0);
#pragma unroll
        for (int i = 0; i < CH_NB; i++) nx2[i] = 0.0;
        if (blk > 1) load(k0 - 2 * CH_NB, CH_NB, nx2);
        __syncthreads();                                         // y carries every later block's update
        if (w0) {
            double y = lane < nb ? yv[k0 + lane] : 0.0;
            const double rd = lane < nb ? rd_all[k0 + lane] : 0.0;
            int ln = lane;
            asm volatile("" : "+v"(ln));                             // (keeps the 64 lane masks below out of spilled scalar registers)
#pragma unroll
            for (int i = CH_NB - 1; i >= 0; i--) {
                const double xl = y * rd;
                const double xi = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(xl), i), __builtin_amdgcn_readlane(__double2loint(xl), i));
                y = ln == i ? xi : (ln < i ? y - cur[i] * xi : y);
            }
            if (lane < CH_NB) s_x[lane] = y;
            if (lane < nb) yv[k0 + lane] = y;
        }
        __syncthreads();
        if (!w0 && t < k0) {
            double acc = yv[t];
#pragma unroll
            for (int i = 0; i < CH_NB; i++) acc -= cur[i] * s_x[i];
            yv[t] = acc;
        }
#pragma unroll
        for (int i = 0; i < CH_NB; i++) { cur[i] = nxt[i]; nxt[i] = nx2[i]; }
    }
    __syncthreads();
}

// lower triangle of S, one thread per entry, many workgroups (latency-bound gathers from H and G)
__device__ __forceinline__ void b_ba_assemble(const BADev &D)
{
    const BACtl *ctl = D.ctl;
    if (ctl->done) return;
    const int n = D.nf, ld = D.nfp;
    const int i = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
    if (j > i) return;                                      // lower triangle only
    const int gi = (i / BA_TILE <= j / BA_TILE) ? i : j, gj = (i / BA_TILE <= j / BA_TILE) ? j : i;   // G holds upper tiles
    double g = 0;
    if (D.det) {                                            // the landmark splits' copies of W^T C W (and of v), in order
        for (int q = 0; q < D.det_ksplit; q++) g += D.Gpart[(size_t)q * ld * ld + (long long)gi * ld + gj];
        if (j == 0) { double t = 0; for (int q = 0; q < D.det_ksplit; q++) t += D.vpart[(size_t)q * ld + i]; D.v[i] = t; }
    } else g = D.G[(long long)gi * ld + gj];
    double val = D.scale_f[i] * D.scale_f[j] * (D.H[(long long)j * ld + i] - g);   // H: upper triangle (j <= i)
    if (i == j) val += D.diag_f[i] / ctl->radius;
    D.S[(long long)i * ld + j] = val;
    (void)n;
}
__global__ __launch_bounds__(256) void k_ba_assemble(BADev D) { b_ba_assemble(D); }
__global__ __launch_bounds__(256) void k_ba_assemble_B(const BADev *__restrict__ arr) { const BADev &D = arr[blockIdx.z]; if ((int)blockIdx.y >= D.nf) return; b_ba_assemble(D); }

__device__ __forceinline__ void b_ba_cholesky(const BADev &D)
{
    BACtl *ctl = D.ctl;
    if (ctl->done) return;
    extern __shared__ __align__(16) unsigned char smem_raw[];
    double *L11 = (double *)smem_raw;                       // CH_NB x CH_LDP : diagonal block / its inverse
    double *yv = L11 + CH_NB * CH_LDP;                      // nfp
    double *P = yv + D.nfp;                                 // (n - CH_NB) x CH_LDP : panel below the diagonal block
    double *rd_all = P + (size_t)((max(0, D.nf - CH_NB) + 15) & ~15) * CH_LDP;   // nfp: reciprocal pivots of all unknowns (backward substitution)
    const int n = D.nf, ld = D.nfp, tid = threadIdx.x, nt = blockDim.x;
    const int wave = tid >> 6, lane = tid & 63;
    __shared__ int s_fail;
    __shared__ double s_red[32][33];
    __shared__ double s_rdiag[CH_NB];                        // 1 / L11[j][j] of the current diagonal block
    __shared__ double s_yk[CH_NB];                           // the block's part of the forward solution (the right-hand side as a panel row)
    double *S = D.S;
    // The right-hand side rides through the factorisation as one more row of the panel: solving its block against L11 IS the
    // forward substitution of that block, and its trailing update (rhs_rest -= P y_blk) replaces the forward pass of the
    // triangular solves (ten blocks of partial sums over L in L2, three barriers each).  Needs a free panel thread.
    const bool rhs_row = n - CH_NB + 1 <= nt - 128;
    // (S was assembled by k_ba_assemble: in here, one workgroup walking the n^2 entries took 85 us of latency)
    for (int i = tid; i < D.nfp; i += nt) yv[i] = i < n ? D.scale_f[i] * (D.bf[i] - D.v[i]) : 0.0;
    if (tid == 0) s_fail = 0;
    __syncthreads();

    unsigned long long tk[6] = {0, 0, 0, 0, 0, 0}, tc = wall_clock64();
#define CH_TICK(i) do { const unsigned long long t_ = wall_clock64(); tk[i] += t_ - tc; tc = t_; } while (0)
    for (int k0 = 0; k0 < n; k0 += CH_NB) {
        const int nb = min(CH_NB, n - k0);
        const int m = n - k0 - nb;                          // rows below the diagonal block
        // (a) diagonal block -> LDS (identity padding when nb < 32), panel rows -> LDS (coalesced)
        for (int e = tid; e < CH_NB * CH_NB; e += nt) {
            const int i = e >> 5, j = e & 31;
            double v = (i == j) ? 1.0 : 0.0;
            if (i < nb && j <= i) v = S[(long long)(k0 + i) * ld + k0 + j];
            L11[i * CH_LDP + j] = v;
        }
        // (eight loads in flight per thread: a load -> LDS store loop pays one L2 round trip per element)
        for (int e0 = tid; e0 < m * CH_NB; e0 += 8 * nt) {
            double v[8];
#pragma unroll
            for (int u = 0; u < 8; u++) {
                const int e = e0 + u * nt, t = e >> 5, j = e & 31;
                v[u] = (e < m * CH_NB && j < nb) ? S[(long long)(k0 + nb + t) * ld + k0 + j] : 0.0;
            }
#pragma unroll
            for (int u = 0; u < 8; u++) {
                const int e = e0 + u * nt;
                if (e < m * CH_NB) P[(e >> 5) * CH_LDP + (e & 31)] = v[u];
            }
        }
        __syncthreads();
        CH_TICK(0);
        // (b) + (c), pipelined through LDS.  Wavefront 0 factors the diagonal block (left-looking, lane i owns row i in
        //     registers, one LDS sync per column) and PUBLISHES its columns in groups of four (L11[.][c], the reciprocal pivots,
        //     then a work-group barrier; a per-column flag with spinning consumers made the register allocator spill the row
        //     arrays).  The other wavefronts solve the panel X L11^T = A21 one row per thread and trail the
        //     factorisation by one column instead of waiting for all 32: the panel solve (9 us per panel as a phase of its own)
        //     hides behind the 5 us pivot chain.
        if (wave == 0) {
            double a[CH_NB];
#pragma unroll
            for (int j = 0; j < CH_NB; j++) a[j] = lane < CH_NB ? L11[lane * CH_LDP + j] : 0.0;
            bool fail = false;
            // (the lane index of THIS panel step: compared against the 32 column numbers below.  Without the laundering the compiler
            // hoists all 64 lane masks out of the panel loop and parks them in spilled scalar registers -- 470 v_writelane / 1000
            // v_readlane with their wait states, on the one wavefront everybody waits for)
            int ln = lane;
            asm volatile("" : "+v"(ln));
            // Column c needs  a[c] - sum_{k<c} a[k] L[c][k]  of every row.  Round 4: the terms of the columns published two
            // barriers ago and earlier (k < 4 (c/4 - 1)) are taken out of the future columns by the HELPER wavefront below, in LDS,
            // while this wavefront works on the current group of four -- it had 90 instructions per column at c = 20, two thirds of
            // them those terms, and every other wavefront of the kernel waits for it.  What stays here: the 4 .. 7 terms of the last
            // two groups (this wavefront's own registers), the same order k = 0, 1, .. as ever (bit-identical factor).  All of them
            // but the last (k = c-1) are known one column earlier and are accumulated while the previous pivot's rsqrt chain is in
            // flight -- except for the first column of a group, whose LDS value is final only after the barrier just passed.
            double pnext = a[0];
#pragma unroll
            for (int c = 0; c < CH_NB; c++) {
                double sacc;
                if ((c & (CH_GRP - 1)) == 0 && c >= 2 * CH_GRP) {
#pragma unroll
                    for (int q = 0; q < CH_GRP; q++) a[c + q] = ln < CH_NB ? L11[ln * CH_LDP + c + q] : 0.0;   // with the helper's terms
                    sacc = a[c];
#pragma unroll
                    for (int k = c - CH_GRP; k < c; k++) sacc -= a[k] * L11[c * CH_LDP + k];
                } else {
                    sacc = pnext;
                    if (c > 0) sacc -= a[c - 1] * L11[c * CH_LDP + c - 1];          // row c of L, final for k < c (broadcast read)
                }
                const double d = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(sacc), c), __builtin_amdgcn_readlane(__double2loint(sacc), c));
                if (c + 1 < CH_NB && !(((c + 1) & (CH_GRP - 1)) == 0 && c + 1 >= 2 * CH_GRP)) {
                    const int kmin = (c + 1) / CH_GRP >= 1 ? CH_GRP * ((c + 1) / CH_GRP - 1) : 0;
                    pnext = a[c + 1];
#pragma unroll
                    for (int k = kmin; k < c; k++) pnext -= a[k] * L11[(c + 1) * CH_LDP + k];
                }
                if (!(d > 0.0) || !isfinite(d)) fail = true;
                // pivot through 1/sqrt(d): v_rsq_f64 seed (~2^-26) + two Newton steps, then L[c][c] = d r with one Heron
                // correction and L[i][c] = sacc r -- 9 dependent instructions instead of the ~25 of sqrt() followed by a
                // division, 32 times per block on the kernel's longest serial chain (and 15 KB less unrolled code)
                double r = __builtin_amdgcn_rsq(d);
                r = fma(0.5 * r, fma(-(d * r), r, 1.0), r);
                r = fma(0.5 * r, fma(-(d * r), r, 1.0), r);
                double dj = d * r;
                dj = fma(0.5 * r, fma(-dj, dj, d), dj);
                const double l = ln == c ? dj : sacc * r;
                a[c] = ln >= c ? l : 0.0;
                if (ln < CH_NB) L11[ln * CH_LDP + c] = a[c];                 // (lanes < c write the 0 of the upper triangle: never read)
                // reciprocal pivot 1 / L[c][c]: r refined by one Newton step of the reciprocal (two FMAs, no division)
                if (ln == c) { const double rc = fma(r, fma(-dj, r, 1.0), r); s_rdiag[c] = rc; rd_all[k0 + c] = rc; }
                wave_lds_sync();
                if ((c & (CH_GRP - 1)) == CH_GRP - 1) __syncthreads();   // columns c-CH_GRP+1 .. c are published: the panel wavefronts may use them
            }
            if (fail && lane == 0) s_fail = 1;
        } else if (wave == 4) {
            // the helper (same SIMD as wavefront 0, no panel rows): before barrier g the columns of the groups < g are published; it
            // takes the terms of group g-1 out of the columns of the groups > g (row per lane, two columns at a time), in place
            const int hi = lane & 31, hh = lane >> 5;
#pragma unroll
            for (int g = 0; g < CH_NB / CH_GRP; g++) {
                if (g >= 1) {
                    const int kb = CH_GRP * (g - 1);
                    double lk4[CH_GRP];
#pragma unroll
                    for (int q = 0; q < CH_GRP; q++) lk4[q] = L11[hi * CH_LDP + kb + q];
#pragma unroll
                    for (int jj = CH_GRP * (g + 1); jj < CH_NB; jj += 2) {
                        const int j = jj + hh;
                        double acc = L11[hi * CH_LDP + j];
#pragma unroll
                        for (int q = 0; q < CH_GRP; q++) acc -= lk4[q] * L11[j * CH_LDP + kb + q];
                        L11[hi * CH_LDP + j] = acc;
                    }
                }
                __syncthreads();
            }
        } else {
            // left-looking per row (x[32] in registers, row j of L read as one contiguous LDS row).  Every panel wavefront
            // passes the same 8 work-group barriers as wavefront 0, whether its threads own a row or not.
            // (wavefronts 1-3 and 5-7 take rows 0 .. 383; two rows per thread on three wavefronts would halve the broadcast reads of
            // L11 -- 1 KB comes back per ds_read_b128 whatever the number of rows it serves -- but x and z together need more
            // than the 256 registers the kernel has: measured with spills, 202 us against 89)
            const int t = wave < 4 ? tid - 64 : tid - 128;
            const bool has = t < m;
            const bool rhs = rhs_row && t == m;                 // the thread after the last panel row takes the right-hand side
            double x[CH_NB];
#pragma unroll
            for (int j = 0; j < CH_NB; j++) x[j] = has ? P[t * CH_LDP + j] : (rhs ? yv[k0 + j] : 0.0);
#pragma unroll
            for (int j = 0; j < CH_NB; j++) {
                if ((j & (CH_GRP - 1)) == 0) {
                    // x[j-1] must be finished BEFORE the barrier: without this artificial use the scheduler drains all eight
                    // barriers first -- loading the whole block into registers (992 VGPRs: spills) -- and computes afterwards,
                    // which also serialises the panel solve behind the factorisation again
                    if (j > 0) asm volatile("" ::"v"(x[j - 1]) : "memory");
                    __syncthreads();                           // columns j .. j+3 of L11 and their reciprocal pivots are there
                }
                double acc = x[j];
#pragma unroll
                for (int k = 0; k < j; k++) acc -= x[k] * L11[j * CH_LDP + k];
                x[j] = acc * s_rdiag[j];
            }
            if (has) {
#pragma unroll
                for (int j = 0; j < CH_NB; j++) P[t * CH_LDP + j] = x[j];
            }
            if (rhs) {
#pragma unroll
                for (int j = 0; j < CH_NB; j++) { s_yk[j] = x[j]; if (j < nb) yv[k0 + j] = x[j]; }
            }
        }
        __syncthreads();
        // rows beyond the pipelined ones (only for reduced systems of more than ~480 unknowns): plain pass on the LDS rows, the
        // block is complete.  Rolled on purpose: an unrolled copy of the 496-term row solve is 12 KB of code, and this kernel has
        // to stay inside the 64 KB instruction cache (round 4: at 77 KB every panel step re-fetched its code from L2).
        for (int t = tid + 384; t < m; t += nt) {
            double *xr = P + t * CH_LDP;
#pragma nounroll
            for (int j = 0; j < CH_NB; j++) {
                double acc = xr[j];
#pragma nounroll
                for (int k = 0; k < j; k++) acc -= xr[k] * L11[j * CH_LDP + k];
                xr[j] = acc * s_rdiag[j];
            }
        }
        __syncthreads();
        if (rhs_row) {
            // trailing update of the right-hand side: rhs[below] -= P y_blk
            for (int i = tid; i < m; i += nt) {
                double acc = yv[k0 + nb + i];
#pragma unroll
                for (int j = 0; j < CH_NB; j++) acc -= P[i * CH_LDP + j] * s_yk[j];
                yv[k0 + nb + i] = acc;
            }
        }
        CH_TICK(1);
        if (s_fail) break;
        // factored block and panel back to HBM (coalesced)
        for (int e = tid; e < nb * nb; e += nt) {
            const int i = e / nb, j = e - i * nb;
            if (j <= i) S[(long long)(k0 + i) * ld + k0 + j] = L11[i * CH_LDP + j];
        }
        for (int e = tid; e < m * CH_NB; e += nt) {
            const int t = e >> 5, j = e & 31;
            if (j < nb) S[(long long)(k0 + nb + t) * ld + k0 + j] = P[t * CH_LDP + j];
        }
        CH_TICK(2);
        // (d) trailing update  A22 -= P P^T  (lower triangle) on the fp64 matrix cores: one wavefront per 16x16 tile,
        //     8 x v_mfma_f64_16x16x4_f64 over the 32 panel columns.  Operand layout (cdna_hip_programming.md, f64 MFMA):
        //     A: lane holds A[lane & 15][lane >> 4], B: lane holds B[lane >> 4][lane & 15] -- both are rows of the LDS
        //     panel --, C/D: col = lane & 15, row = (lane >> 4) + 4 * reg.  S stays in HBM/L2; a tile is read, updated
        //     and written once per panel step.
        {
            typedef double d4 __attribute__((ext_vector_type(4)));
            const int mb = (m + 15) >> 4, nwv = nt >> 6;
            const int lr = lane & 15, lk = lane >> 4;
            // A wavefront takes the tiles wv, wv + nwv, .. of the row-major lower-triangle enumeration, two at a time (two
            // independent MFMA chains).  Round 4: the phase was a SUM of its parts (knock-outs: 24 us of tile bookkeeping -- a
            // double-precision sqrt per tile index, 64-bit multiplies per element address, four predicates per element --, 31 us of
            // MFMA, 9 us of loads, 6 us of LDS reads, 4 us of stores; two wavefronts per SIMD overlap little).  Now the tile
            // walk is integer arithmetic on the scalar unit (wave-uniform), an element's address is a uniform base + one of four
            // per-lane constants, operand rows are read unpredicated (garbage rows >= m only reach rows / columns that are not
            // stored), and the old values of the next pair are requested before the chains of the current pair run.
            const int ntile = mb * (mb + 1) / 2;
            const int wv = __builtin_amdgcn_readfirstlane(wave);
            auto advance = [&](int &bi, int &bj, int step) { bj += step; while (bj > bi) { bj -= bi + 1; bi++; } };
            int lo[4];                                              // element (lk + 4 r, lr) of a tile, in doubles from the tile's corner
#pragma unroll
            for (int r = 0; r < 4; r++) lo[r] = (lk + 4 * r) * ld + lr;
            double *Sc = S + (long long)(k0 + nb) * ld + k0 + nb;      // corner of the trailing matrix
            const double *Pl = P + lr * CH_LDP + lk;                   // this lane's operand element of tile row 0
            auto corner = [&](int bi, int bj) { return Sc + ((long long)bi * ld + bj) * 16; };
            auto okmask = [&](int bi, int bj, int r) { return (16 * bi + lk + 4 * r < m) && (bi != bj || lr <= lk + 4 * r); };
            auto fetch = [&](int bi, int bj, bool has, double (&o)[4]) {
                const double *c = corner(bi, bj);
#pragma unroll
                for (int r = 0; r < 4; r++) o[r] = (has && okmask(bi, bj, r)) ? c[lo[r]] : 0.0;
            };
            int bi0 = 0, bj0 = 0, bi1, bj1;
            advance(bi0, bj0, wv);
            bi1 = bi0; bj1 = bj0; advance(bi1, bj1, nwv);
            double old0[4], old1[4];
            fetch(bi0, bj0, wv < ntile, old0);
            fetch(bi1, bj1, wv + nwv < ntile, old1);
            for (int t0 = wv; t0 < ntile; t0 += 2 * nwv) {
                const bool has1 = t0 + nwv < ntile;
                int nbi0 = bi1, nbj0 = bj1, nbi1, nbj1;
                advance(nbi0, nbj0, nwv);
                nbi1 = nbi0; nbj1 = nbj0; advance(nbi1, nbj1, nwv);
                double nold0[4], nold1[4];
                fetch(nbi0, nbj0, t0 + 2 * nwv < ntile, nold0);
                fetch(nbi1, nbj1, t0 + 3 * nwv < ntile, nold1);
                const double *pa0 = Pl + bi0 * (16 * CH_LDP), *pb0 = Pl + bj0 * (16 * CH_LDP);
                const double *pa1 = Pl + (has1 ? bi1 : bi0) * (16 * CH_LDP), *pb1 = Pl + (has1 ? bj1 : bj0) * (16 * CH_LDP);
                d4 c0 = {0., 0., 0., 0.}, c1 = {0., 0., 0., 0.};
#pragma unroll
                for (int kk = 0; kk < CH_NB / 4; kk++) {
                    c0 = __builtin_amdgcn_mfma_f64_16x16x4f64(pa0[4 * kk], pb0[4 * kk], c0, 0, 0, 0);
                    c1 = __builtin_amdgcn_mfma_f64_16x16x4f64(pa1[4 * kk], pb1[4 * kk], c1, 0, 0, 0);
                }
                double *q0 = corner(bi0, bj0), *q1 = corner(bi1, bj1);
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    if (okmask(bi0, bj0, r)) q0[lo[r]] = old0[r] - c0[r];
                    if (has1 && okmask(bi1, bj1, r)) q1[lo[r]] = old1[r] - c1[r];
                }
                bi0 = nbi0; bj0 = nbj0; bi1 = nbi1; bj1 = nbj1;
#pragma unroll
                for (int r = 0; r < 4; r++) { old0[r] = nold0[r]; old1[r] = nold1[r]; }
            }
        }
        __syncthreads();
        CH_TICK(3);
    }
    if (s_fail) { if (tid == 0) ctl->lin_fail = 1; return; }

    CH_TICK(4);
    // forward substitution rode along as a panel row (rhs_row: the host sends systems of more than 479 unknowns to the HBM path);
    // backward substitution from the factor itself -- no inverse diagonal blocks (rounds 1-3 computed them here: 20 us and 12 KB of
    // unrolled code in a kernel that has to fit the instruction cache)
    chol_backward_blocks(D, yv, rd_all, &s_red[0][0]);

    for (int i = tid; i < n; i += nt) D.yf[i] = yv[i];
    CH_TICK(5);
    if (tid == 0) for (int i = 0; i < 6; i++) ctl->dbg[i] = tk[i];
#undef CH_TICK
}
__global__ __launch_bounds__(512) void k_ba_cholesky(BADev D) { b_ba_cholesky(D); }
__global__ __launch_bounds__(512) void k_ba_cholesky_B(const BADev *__restrict__ arr) { const BADev &D = arr[blockIdx.z]; b_ba_cholesky(D); }

// ================================================================================== pose-only problems in ONE kernel
// MultiViewGeometry::ceresPnP (src/multi_view_geometry.cpp:492-586): one free pose, a few hundred fixed world points.  The
// multi-kernel loop above costs ~10 launches of ~6 us per LM iteration whatever the problem size -- 0.45 ms per solve, four times
// what one CPU core needs.  Here the whole trust-region loop runs in ONE work-group: residual blocks over the threads, the
// 6 x 6 normal equations in LDS, the scalar bookkeeping through the same d_ctl_* functions as the multi-kernel path.
// Used when the problem has no landmarks, pose-only residual blocks and exactly one optimised keyframe (ba_run).
__global__ __launch_bounds__(256) void k_ba_pose_only(BADev D, BAOpt O, BACtl ctl0)
{
    __shared__ BACtl cl;
    __shared__ double s_H[21], s_b[6], s_cost, s_scale[6], s_diag[6], s_y[6];
    __shared__ double s_x[7], s_xRT[12], s_c[7], s_cRT[12];      // the optimised pose and its candidate stay in LDS (+ cached R | t)
    __shared__ int s_kf, s_flag;
    const int tid = threadIdx.x, nt = blockDim.x;
    if (tid == 0) {
        cl = ctl0;
        int kf = 0;
        for (int k = 0; k < D.n_kf; k++) if (D.pose_col[k] == 0) kf = k;
        s_kf = kf;
    }
    if (tid < 6) { s_scale[tid] = 1.0; s_diag[tid] = 0.0; s_y[tid] = 0.0; }
    for (int k = tid; k < D.n_kf; k += nt) d_pose_to_RT(D.x_pose + 7 * k, D.x_RT + 12 * k);      // (constant keyframes are read from here)
    __threadfence_block();
    __syncthreads();
    const int kf = s_kf;
    if (tid == 0) { for (int c = 0; c < 7; c++) s_x[c] = D.x_pose[7 * kf + c]; d_pose_to_RT(s_x, s_xRT); }
    __syncthreads();
    double *xp = s_x, *cp = s_c;
    auto RTx = [&](int o) -> const double * { return o == kf ? s_xRT : D.x_RT + 12 * o; };
    auto RTc = [&](int o) -> const double * { return o == kf ? s_cRT : D.x_RT + 12 * o; };      // constant keyframes: candidate = x

    // J^T J (upper triangle, 21), J^T r (6) and the robustified cost at x (k_ba_linearize_po)
    auto linearize = [&]() {
        if (tid < 21) s_H[tid] = 0;
        if (tid < 6) s_b[tid] = 0;
        if (tid == 0) s_cost = 0;
        __syncthreads();
        double cost = 0, h[21], b[6];
        for (int q = 0; q < 21; q++) h[q] = 0;
        for (int q = 0; q < 6; q++) b[q] = 0;
        for (int k = tid; k < D.n_po; k += nt) {
            const int o = D.po_kf[k], co = D.pose_col[o];
            double r[2], Jo[12];
            const int dp = d_residual_pnp<true>(D, RTx(o), D.po_xyz + 3 * k, D.po_uv + 2 * k, D.po_sigma[k], r, Jo);
            const double sq = r[0] * r[0] + r[1] * r[1];
            const int orig = D.po_orig[k];
            D.chi2[orig] = sq; D.dpos[orig] = (uint8_t)dp;
            double rho0, rho1;
            d_huber(D.huber, sq, rho0, rho1);
            cost += 0.5 * rho0;
            if (co < 0) continue;
            const double sc = sqrt(rho1);
            r[0] *= sc; r[1] *= sc;
            for (int q = 0; q < 12; q++) Jo[q] *= sc;
            int t = 0;
            for (int c = 0; c < 6; c++) {
                b[c] += Jo[c] * r[0] + Jo[6 + c] * r[1];
                for (int d = c; d < 6; d++) h[t++] += Jo[c] * Jo[d] + Jo[6 + c] * Jo[6 + d];
            }
        }
        // wavefront sums first (27 + 1 values), then one LDS atomic per wavefront and value
        for (int q = 0; q < 21; q++) { const double v = wave_sum(h[q]); if ((tid & 63) == 0 && v != 0.0) atomicAdd(&s_H[q], v); }
        for (int q = 0; q < 6; q++) { const double v = wave_sum(b[q]); if ((tid & 63) == 0 && v != 0.0) atomicAdd(&s_b[q], v); }
        cost = wave_sum(cost);
        if ((tid & 63) == 0 && cost != 0.0) atomicAdd(&s_cost, cost);
        __syncthreads();
        if (tid == 0) { cl.cost_acc += s_cost; cl.need_lin = 0; cl.fresh_lin = 1; }       // (a linearisation at x is now available)
        __syncthreads();
    };
    auto Hd = [&](int i, int j) { const int a = i < j ? i : j, bq = i < j ? j : i; return s_H[a * 6 - a * (a - 1) / 2 + (bq - a)]; };   // upper-packed

    linearize();
    for (int it = 0; it <= O.max_iter; it++) {
        // ---- k_ba_iter_begin ----
        if (tid == 0) {
            const int fresh = cl.fresh_lin;
            double gm = 0;
            if (fresh) {
                if (O.jacobi && !cl.scaled) for (int c = 0; c < 6; c++) s_scale[c] = 1.0 / (1.0 + sqrt(Hd(c, c)));
                double d[6], out[7];
                for (int c = 0; c < 6; c++) d[c] = -s_b[c];
                d_se3_left_plus(xp, d, out);
                for (int c = 0; c < 7; c++) gm = fmax(gm, fabs(xp[c] - out[c]));
            }
            d_ctl_iter_begin(cl, O, fresh, gm);
            if (!cl.done) {
                if (!cl.reuse_diag) for (int c = 0; c < 6; c++) s_diag[c] = fmin(fmax(s_scale[c] * s_scale[c] * Hd(c, c), O.min_diag), O.max_diag);
                cl.reuse_diag = 1;
                // ---- k_ba_assemble + Cholesky + the two triangular solves on the 6 x 6 system ----
                double L[6][6], y[6];
                bool fail = false;
                for (int i = 0; i < 6; i++)
                    for (int j = 0; j <= i; j++) L[i][j] = s_scale[i] * s_scale[j] * Hd(i, j) + (i == j ? s_diag[i] / cl.radius : 0.0);
                for (int j = 0; j < 6; j++) {
                    double dsum = L[j][j];
                    for (int k = 0; k < j; k++) dsum -= L[j][k] * L[j][k];
                    if (!(dsum > 0.0) || !isfinite(dsum)) { fail = true; break; }
                    const double ljj = sqrt(dsum);
                    L[j][j] = ljj;
                    for (int i = j + 1; i < 6; i++) {
                        double v = L[i][j];
                        for (int k = 0; k < j; k++) v -= L[i][k] * L[j][k];
                        L[i][j] = v / ljj;
                    }
                }
                if (fail) cl.lin_fail = 1;
                else {
                    for (int i = 0; i < 6; i++) { double v = s_scale[i] * s_b[i]; for (int k = 0; k < i; k++) v -= L[i][k] * y[k]; y[i] = v / L[i][i]; }
                    for (int i = 5; i >= 0; i--) { double v = y[i]; for (int k = i + 1; k < 6; k++) v -= L[k][i] * y[k]; y[i] = v / L[i][i]; }
                    for (int i = 0; i < 6; i++) s_y[i] = y[i];
                }
                // ---- k_ba_candidate ----
                int ok = !cl.lin_fail;
                double P1 = 0, P2 = 0;
                if (ok)
                    for (int i = 0; i < 6; i++) {
                        const double yi = s_y[i], si = s_scale[i];
                        if (!isfinite(yi)) ok = 0;
                        P1 += yi * si * s_b[i];
                        P2 += yi * si * s_b[i] - (s_diag[i] / cl.radius) * yi * yi;
                    }
                const int valid = d_ctl_candidate(cl, O, ok, P1, P2);
                if (valid) {
                    double d[6], out[7];
                    for (int c = 0; c < 6; c++) d[c] = -s_y[c] * s_scale[c];
                    d_se3_left_plus(xp, d, out);
                    for (int c = 0; c < 7; c++) cp[c] = out[c];
                    d_pose_to_RT(out, s_cRT);
                }
                s_flag = valid;
            } else s_flag = -1;
            s_cost = 0;
        }
        __threadfence_block();
        __syncthreads();
        if (s_flag < 0) break;                                  // terminated in the bookkeeping
        if (s_flag == 0) continue;                              // invalid step: radius already shrunk, same linearisation
        // ---- k_ba_cost at the candidate (also the N4 outputs) ----
        double cost = 0;
        for (int k = tid; k < D.n_po; k += nt) {
            double r[2];
            const int dp = d_residual_pnp<false>(D, RTc(D.po_kf[k]), D.po_xyz + 3 * k, D.po_uv + 2 * k, D.po_sigma[k], r, nullptr);
            const double sq = r[0] * r[0] + r[1] * r[1];
            const int orig = D.po_orig[k];
            D.chi2[orig] = sq; D.dpos[orig] = (uint8_t)dp;
            double rho0, rho1;
            d_huber(D.huber, sq, rho0, rho1);
            cost += 0.5 * rho0;
        }
        cost = wave_sum(cost);
        if ((tid & 63) == 0 && cost != 0.0) atomicAdd(&s_cost, cost);
        __syncthreads();
        // ---- k_ba_decide ----
        if (tid == 0) {
            cl.cost_acc += s_cost;
            double SN = 0, XN = 0;
            for (int c = 0; c < 7; c++) { const double d = xp[c] - cp[c]; SN += d * d; XN += cp[c] * cp[c]; }
            const int accept = d_ctl_decide(cl, O, SN, XN);
            if (accept) { for (int c = 0; c < 7; c++) xp[c] = cp[c]; for (int c = 0; c < 12; c++) s_xRT[c] = s_cRT[c]; }
            s_flag = cl.done ? -1 : (cl.need_lin ? 1 : 0);
        }
        __threadfence_block();
        __syncthreads();
        if (s_flag < 0) break;
        if (s_flag == 1) linearize();
    }
    if (tid == 0) { *D.ctl = cl; for (int c = 0; c < 7; c++) D.x_pose[7 * kf + c] = s_x[c]; }
}

// ================================================================================== big path (BADev::big)
// clears what the big-path lineariser accumulates into (k_ba_decide leaves H alone on this path: one work-group clearing
// nfp^2 doubles took 150 us at 300 keyframes)
__global__ __launch_bounds__(256) void k_ba_zero_lin(BADev D)
{
    const BACtl *ctl = D.ctl;
    if (ctl->done || !ctl->need_lin) return;
    const long long nh = (long long)D.nfp * D.nfp, nw = (long long)6 * D.n_cw, stride = (long long)gridDim.x * blockDim.x;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < nh; e += stride) D.H[e] = 0;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < nw; e += stride) D.cww[e] = 0;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < D.nfp; e += stride) D.bf[e] = 0;
}

// W^T C W and W^T (c E^T b) from the SPARSE W.  G = sum_l c_l w_l w_l^T with w_l the landmark's slots; the row block of one
// keyframe (6 x nfp doubles, <= 96 KB) is accumulated in LDS by the work-group(s) that own the keyframe: a wavefront takes one
// of the keyframe's slots (landmark l, block w_i), stages the landmark's slot list (columns + blocks, <= 64 at a time) in its
// LDS scratch, and lane (j, b) adds c w_i[a] w_j[b] for a = 0..5 with LDS fp64 atomics.  Only the blocks k_ba_assemble reads
// are computed (tile of the column >= tile of the row, i.e. roughly the upper half: work-groups are issued first rows first,
// longest first).  nsplit > 1 (few keyframes): several work-groups share a row block and flush it with global atomics.
// First version: one wavefront per landmark, lane per entry, 36 E^2 GLOBAL atomics per landmark -- 44 ms per iteration on the
// 50 KF x 10 k x 30 stereo problem, 50 ms at 300 KF (profiles/archive/r2_ba_big_*).
#define SS_WAVES 8
// Beyond 341 keyframes the row block no longer fits the LDS: blockIdx.y walks over column chunks of `ncol` columns (a multiple of
// 6: pose blocks never straddle a chunk); a work-group accumulates the part [col0, col0 + ncol) of its row block only, and the
// chunk that holds no column >= cmin exits at once.
__global__ __launch_bounds__(64 * SS_WAVES) void k_ba_schur_sparse(BADev D, int nsplit, int ncol)
{
    const BACtl *ctl = D.ctl;
    if (ctl->done) return;
    extern __shared__ __align__(16) unsigned char smem_raw[];
    const int nfp = D.nfp, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int col0 = blockIdx.y * ncol, ncw = min(ncol, nfp - col0);      // this work-group's columns
    double *R = (double *)smem_raw;                                       // 6 x ncol
    double *wsc = R + 6 * ncol + wave * (64 * 6);                         // this wavefront's staged slot blocks
    int *csc = (int *)(R + 6 * ncol + SS_WAVES * 64 * 6) + wave * 64;     // ... and their columns
    __shared__ double vacc[6];
    const int ob = blockIdx.x / nsplit, sp = blockIdx.x - ob * nsplit, ci = 6 * ob;
    const int cmin = (ci / BA_TILE) * BA_TILE - 5;                        // blocks entirely left of the row's first tile are never read
    if (col0 + ncw + 5 <= cmin) return;                                   // (uniform) nothing of this chunk is ever read
    const bool own_v = ci >= col0 && ci < col0 + ncw;                     // W^T (c E^T b): added once, by the chunk of the diagonal block
    for (int e = threadIdx.x; e < 6 * ncol; e += blockDim.x) R[e] = 0;
    if (threadIdx.x < 6) vacc[threadIdx.x] = 0;
    __syncthreads();
    const int b0 = D.kfl_ptr[ob], b1 = D.kfl_ptr[ob + 1];
    const int len = (b1 - b0 + nsplit - 1) / nsplit, e0 = b0 + sp * len, e1 = min(b1, e0 + len);
    double dv = 0;
    for (int e = e0 + wave; e < e1; e += SS_WAVES) {
        const int slot = D.kfl_idx[e], lm = D.cw_lm[slot];
        const double c = D.cl[lm], ce = c * D.etb[lm];
        const int j0 = D.cw_ptr[lm], j1 = D.cw_ptr[lm + 1];
        double wi[6];
        for (int q = 0; q < 6; q++) wi[q] = D.cww[(long long)6 * slot + q];
        if (lane < 6 && own_v) dv += ce * D.cww[(long long)6 * slot + lane];
        for (int jb = j0; jb < j1; jb += 64) {
            const int j = jb + lane, nj = min(64, j1 - jb);
            wave_lds_sync();
            if (j < j1) {
                csc[lane] = D.cw_col[j];
                for (int q = 0; q < 6; q++) wsc[lane * 6 + q] = D.cww[(long long)6 * j + q];
            }
            wave_lds_sync();
            for (int t = lane; t < nj * 6; t += 64) {
                const int jj = t / 6, b = t - jj * 6, cj = csc[jj];
                if (cj < cmin || cj < col0 || cj >= col0 + ncw) continue;
                const double wjb = c * wsc[t];
                double *dst = R + (cj - col0) + b;
#pragma unroll
                for (int a = 0; a < 6; a++) atomicAdd(&dst[a * ncol], wi[a] * wjb);
            }
        }
    }
    if (lane < 6 && dv != 0.0) atomicAdd(&vacc[lane], dv);
    __syncthreads();
    for (int e = threadIdx.x; e < 6 * ncol; e += blockDim.x) {
        const double v = R[e];
        if (v == 0.0) continue;
        const int a = e / ncol, col = col0 + (e - a * ncol);
        double *g = &D.G[(long long)(ci + a) * nfp + col];
        if (nsplit == 1) *g = v; else atomicAdd(g, v);
    }
    if (threadIdx.x < 6 && vacc[threadIdx.x] != 0.0) atomicAdd(&D.v[ci + threadIdx.x], vacc[threadIdx.x]);
}

// Blocked right-looking Cholesky of the reduced system on HBM, three kernels per 32-column panel:
//   k_chol_diag  (1 wavefront): factor the diagonal block in LDS (same register-row algorithm as k_ba_cholesky), write it back, and
//                its inverse (for the triangular solves) to Linv
//   k_chol_panel (64 rows per work-group): X L11^T = A21 by substitution, one row per thread
//   k_chol_trail (one 32 x 32 tile per work-group, lower triangle): A22 -= X X^T
// then k_chol_solve (1 work-group): the two triangular solves.  ~3 * nf / 32 launches per LM iteration: this path is for the
// loop-closure / offline BAs (hundreds of keyframes), where a solve takes milliseconds either way.
__global__ __launch_bounds__(64) void k_chol_diag(BADev D, int k0)
{
    BACtl *ctl = D.ctl;
    if (ctl->done || ctl->lin_fail) return;
    __shared__ double L11[CH_NB * CH_LDP];
    const int n = D.nf, ld = D.nfp, lane = threadIdx.x;
    const int nb = min(CH_NB, n - k0);
    double *S = D.S;
    for (int e = lane; e < CH_NB * CH_NB; e += 64) {
        const int i = e >> 5, j = e & 31;
        double v = (i == j) ? 1.0 : 0.0;
        if (i < nb && j <= i) v = S[(long long)(k0 + i) * ld + k0 + j];
        L11[i * CH_LDP + j] = v;
    }
    wave_lds_sync();
    double a[CH_NB];
#pragma unroll
    for (int j = 0; j < CH_NB; j++) a[j] = lane < CH_NB ? L11[lane * CH_LDP + j] : 0.0;
    bool fail = false;
    double pnext = a[0];
#pragma unroll
    for (int c = 0; c < CH_NB; c++) {
        double sacc = pnext;
        if (c > 0) sacc -= a[c - 1] * L11[c * CH_LDP + c - 1];
        const double d = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(sacc), c), __builtin_amdgcn_readlane(__double2loint(sacc), c));
        if (c + 1 < CH_NB) {
            pnext = a[c + 1];
#pragma unroll
            for (int k = 0; k < c; k++) pnext -= a[k] * L11[(c + 1) * CH_LDP + k];
        }
        if (!(d > 0.0) || !isfinite(d)) fail = true;
        double r = __builtin_amdgcn_rsq(d);
        r = fma(0.5 * r, fma(-(d * r), r, 1.0), r);
        r = fma(0.5 * r, fma(-(d * r), r, 1.0), r);
        double dj = d * r;
        dj = fma(0.5 * r, fma(-dj, dj, d), dj);
        const double l = lane == c ? dj : sacc * r;
        a[c] = lane >= c ? l : 0.0;
        if (lane >= c && lane < CH_NB) L11[lane * CH_LDP + c] = a[c];
        if (lane == c) L11[c * CH_LDP + CH_NB] = fma(r, fma(-dj, r, 1.0), r);          // reciprocal pivot in the padding column
        wave_lds_sync();
    }
    if (__builtin_amdgcn_ballot_w64(fail) != 0) { if (lane == 0) ctl->lin_fail = 1; return; }
    for (int e = lane; e < nb * nb; e += 64) {
        const int i = e / nb, j = e - i * nb;
        if (j <= i) S[(long long)(k0 + i) * ld + k0 + j] = L11[i * CH_LDP + j];
    }
    if (lane < CH_NB) {                                                 // inverse block: lane j solves L x = e_j
        double x[CH_NB];
#pragma unroll
        for (int i = 0; i < CH_NB; i++) {
            double acc = (i == lane) ? 1.0 : 0.0;
#pragma unroll
            for (int k = 0; k < i; k++) acc -= L11[i * CH_LDP + k] * x[k];
            x[i] = i < lane ? 0.0 : acc * L11[i * CH_LDP + CH_NB];
        }
        double *dst = D.Linv + (long long)(k0 / CH_NB) * CH_NB * CH_NB;
#pragma unroll
        for (int i = 0; i < CH_NB; i++) dst[i * CH_NB + lane] = x[i];
    }
}

__global__ __launch_bounds__(64) void k_chol_panel(BADev D, int k0)
{
    const BACtl *ctl = D.ctl;
    if (ctl->done || ctl->lin_fail) return;
    __shared__ double L11[CH_NB * CH_LDP];
    __shared__ double X[64 * CH_LDP];                                   // the work-group's 64 panel rows (a thread's row stays in LDS: the fully
                                                                        // unrolled register version made the scheduler hoist all 496 loads of L11
                                                                        // -- 512 VGPRs, 624 spills -- and miscomputed from column 12 on)
    const int n = D.nf, ld = D.nfp, lane = threadIdx.x;
    const int nb = min(CH_NB, n - k0), m = n - k0 - nb;
    double *S = D.S;
    for (int e = lane; e < CH_NB * CH_NB; e += 64) {
        const int i = e >> 5, j = e & 31;
        double v = (i == j) ? 1.0 : 0.0;
        if (i < nb && j <= i) v = S[(long long)(k0 + i) * ld + k0 + j];
        L11[i * CH_LDP + j] = v;
    }
    const int t0 = blockIdx.x * 64;
    for (int e = lane; e < 64 * CH_NB; e += 64) {                       // coalesced: 32 consecutive columns of one row per half wavefront
        const int r = e >> 5, j = e & 31;
        X[r * CH_LDP + j] = (t0 + r < m && j < nb) ? S[(long long)(k0 + nb + t0 + r) * ld + k0 + j] : 0.0;
    }
    __syncthreads();
    double *x = X + lane * CH_LDP;
    for (int j = 0; j < CH_NB; j++) {
        double acc = x[j];
        const double *lr = L11 + j * CH_LDP;
        for (int k = 0; k < j; k++) acc -= x[k] * lr[k];
        x[j] = acc / lr[j];
    }
    __syncthreads();
    for (int e = lane; e < 64 * CH_NB; e += 64) {
        const int r = e >> 5, j = e & 31;
        if (t0 + r < m && j < nb) S[(long long)(k0 + nb + t0 + r) * ld + k0 + j] = X[r * CH_LDP + j];
    }
}

__global__ __launch_bounds__(256) void k_chol_trail(BADev D, int k0)
{
    const BACtl *ctl = D.ctl;
    if (ctl->done || ctl->lin_fail) return;
    __shared__ double A[32][33], B[32][33];
    const int n = D.nf, ld = D.nfp, tid = threadIdx.x;
    const int nb = min(CH_NB, n - k0), m = n - k0 - nb;
    // lower-triangular tile index -> (bi, bj), bj <= bi
    int t = blockIdx.x, bi = 0;
    while (t > bi) { t -= bi + 1; bi++; }
    const int bj = t;
    double *S = D.S;
    for (int e = tid; e < 32 * 32; e += 256) {
        const int r = e >> 5, c = e & 31;
        const int ia = bi * 32 + r, ib = bj * 32 + r;
        A[r][c] = (ia < m && c < nb) ? S[(long long)(k0 + nb + ia) * ld + k0 + c] : 0.0;
        B[r][c] = (ib < m && c < nb) ? S[(long long)(k0 + nb + ib) * ld + k0 + c] : 0.0;
    }
    __syncthreads();
    const int r0 = (tid >> 4) * 2, c0 = (tid & 15) * 2;                 // 2 x 2 outputs per thread
    double acc[2][2] = {{0, 0}, {0, 0}};
    for (int k = 0; k < 32; k++) {
        const double a0 = A[r0][k], a1 = A[r0 + 1][k], b0 = B[c0][k], b1 = B[c0 + 1][k];
        acc[0][0] += a0 * b0; acc[0][1] += a0 * b1; acc[1][0] += a1 * b0; acc[1][1] += a1 * b1;
    }
    for (int i = 0; i < 2; i++)
        for (int j = 0; j < 2; j++) {
            const int gi = bi * 32 + r0 + i, gj = bj * 32 + c0 + j;
            if (gi < m && gj <= gi) S[(long long)(k0 + nb + gi) * ld + k0 + nb + gj] -= acc[i][j];
        }
}

__global__ __launch_bounds__(512) void k_chol_solve(BADev D)
{
    const BACtl *ctl = D.ctl;
    if (ctl->done || ctl->lin_fail) return;
    extern __shared__ __align__(16) unsigned char smem_raw[];
    double *L11 = (double *)smem_raw;                       // CH_NB x CH_LDP
    double *yv = L11 + CH_NB * CH_LDP;                      // nfp
    __shared__ double s_red[32][33];
    const int n = D.nf, tid = threadIdx.x, nt = blockDim.x;
    for (int i = tid; i < D.nfp; i += nt) yv[i] = i < n ? D.scale_f[i] * (D.bf[i] - D.v[i]) : 0.0;
    __syncthreads();
    chol_trisolve(D, L11, yv, s_red);
    for (int i = tid; i < n; i += nt) D.yf[i] = yv[i];
}

// ---------------------------------------------------------------------------------- back substitution
// one wavefront per landmark: t_l = W_l . (s .* yf); y_l = s_l (etb_l - t_l) / etep_l
__device__ __forceinline__ void b_ba_backsub(const BADev &D)
{
    BACtl *ctl = D.ctl;
    if (ctl->done) return;
    // G = W^T C W was consumed by k_ba_assemble: clear it for the next iteration's Schur kernels here (many work-groups) instead
    // of a memset launch per iteration
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < (long long)D.nfp * D.nfp; e += (long long)gridDim.x * blockDim.x) D.G[e] = 0;
    const double radius = ctl->radius;
    const int reuse = ctl->reuse_now;
    if (ctl->lin_fail) {
        // (no step: but the LM diagonal of this linearisation has to be on record for the retry that reuses it)
        if (!D.big && !reuse)
            for (int l = blockIdx.x * blockDim.x + threadIdx.x; l < D.n_lm; l += gridDim.x * blockDim.x) { double dg; if (d_lm_c(D, l, radius, 0, &dg) != 0.0) D.diag_l[l] = dg; }
        return;
    }
    extern __shared__ __align__(16) unsigned char smem_raw[];
    double *sy = (double *)smem_raw;                        // s_j * yf_j
    for (int c = threadIdx.x; c < D.nfp; c += blockDim.x) sy[c] = c < D.nf ? D.scale_f[c] * D.yf[c] : 0.0;
    __syncthreads();
    // Sixteen lanes per landmark, four landmarks per wavefront (round 4; a wavefront per landmark walked its ~5 landmarks one after
    // the other, each a 300-term dot product, a 6-step wave reduction and a tail of dependent scalar loads in lane 0: 32 us).  The
    // lane that finishes a landmark also forms its candidate x - s y and the landmark's share of the step norms and of the finite
    // check: the one-work-group kernels k_ba_candidate / k_ba_decide no longer walk the landmarks.
    const int lane = threadIdx.x & 63, l16 = lane & 15, wave = threadIdx.x >> 6;
    double a1 = 0, a2 = 0, a3 = 0, sn = 0, xn = 0;
    int bad = 0;
    for (int base = blockIdx.x * 16; base < D.n_lm; base += gridDim.x * 16) {
        const int lm = base + 4 * wave + (lane >> 4);
        const bool in = lm < D.n_lm;
        const bool has = in && d_lm_has(D, lm);
        double t = 0;
        if (has) {
            if (D.big) {
                // sparse W: the landmark's slots
                for (int j = D.cw_ptr[lm] + l16; j < D.cw_ptr[lm + 1]; j += 16) {
                    const int col = D.cw_col[j];
                    const double *w = D.cww + (long long)6 * j;
                    for (int q = 0; q < 6; q++) t += w[q] * sy[col + q];
                }
            } else {
                const double *wr = D.W + (long long)lm * D.nfp;
#pragma unroll 4
                for (int c = l16; c < D.nfp; c += 16) t += wr[c] * sy[c];
            }
        }
        t += __shfl_xor(t, 8, 64); t += __shfl_xor(t, 4, 64); t += __shfl_xor(t, 2, 64); t += __shfl_xor(t, 1, 64);
        if (l16 == 0 && in) {
            const double x = D.x_lam[lm];
            if (!has) { D.yl[lm] = 0; D.c_lam[lm] = x; }
            else {
                const double s = D.scale_l[lm], ete = D.ete[lm], etb = D.etb[lm];
                double dg = 0;
                const double c = D.big ? D.cl[lm] : d_lm_c(D, lm, radius, reuse, &dg);      // s^2 / etep
                if (!D.big && !reuse) D.diag_l[lm] = dg;       // (kept for the iterations that reuse it)
                const double y = (c / s) * (etb - t);          // s (etb - t) / etep
                D.yl[lm] = y;
                a1 += y * s * etb;
                a2 += 2.0 * y * s * t + s * s * ete * y * y;
                a3 += c * t * t;                               // y_f^T G' y_f  (G' = scaled W^T C W)
                const double cand = x - y * s;                 // candidate = Plus(x, step .* scale), step = -y
                D.c_lam[lm] = cand;
                if (!isfinite(y)) bad = 1;
                sn += (x - cand) * (x - cand); xn += cand * cand;
            }
        }
    }
    __shared__ double s_part[4];
    a1 = block_sum(a1, s_part); a2 = block_sum(a2, s_part); a3 = block_sum(a3, s_part);
    sn = block_sum(sn, s_part); xn = block_sum(xn, s_part);
    const int anybad = __syncthreads_or(bad);
    if (threadIdx.x == 0) {
        double *pt = D.part + blockIdx.x;
        pt[0] = a1; pt[BA_PART_MAX] = a2; pt[2 * BA_PART_MAX] = a3; pt[3 * BA_PART_MAX] = sn; pt[4 * BA_PART_MAX] = xn;
        if (anybad) atomicOr(&ctl->bad_step, 1);
    }
}
__global__ __launch_bounds__(256) void k_ba_backsub(BADev D) { b_ba_backsub(D); }
__global__ __launch_bounds__(256) void k_ba_backsub_B(const BADev *__restrict__ arr) { const BADev &D = arr[blockIdx.z]; b_ba_backsub(D); }

// ---------------------------------------------------------------------------------- candidate (1 block)
__device__ __forceinline__ void b_ba_candidate(const BADev &D, BAOpt O)
{
    BACtl *ctl = D.ctl;
    if (ctl->done) return;
    __shared__ double s_part[3][16];
    __shared__ int s_flag;
    const int tid = threadIdx.x, nt = blockDim.x;
    int ok = !ctl->lin_fail;
    // yf . g'_f ; yf^T H'_pp yf from the solved system (S y = rhs, S = H' - G' + D^2):
    //   y^T H' y = y . rhs + y^T G' y - sum_i D_i^2 y_i^2   with y^T G' y = sum_l c_l t_l^2 (k_ba_backsub)
    double p1 = 0, p2 = 0; int bad = 0;
    if (ok) {
        const double radius = ctl->radius;
        for (int i = tid; i < D.nf; i += nt) {
            const double yi = D.yf[i], si = D.scale_f[i];
            if (!isfinite(yi)) bad = 1;
            p1 += yi * si * D.bf[i];
            p2 += yi * si * (D.bf[i] - D.v[i]) - (D.diag_f[i] / radius) * yi * yi;
        }
        if (D.ldim == 1) bad |= ctl->bad_step;                 // (k_ba_backsub looked at every landmark step)
        else {
#pragma unroll 4
            for (int l = tid; l < D.n_lm * D.ldim; l += nt) if (!isfinite(D.yl[l])) bad = 1;
        }
    }
    double P1 = p1, P2 = p2, nbad = (double)bad;
    block_reduce3<false>(P1, P2, nbad, s_part);
    if (nbad > 0) ok = 0;                                  // (thread 0 only: the only consumer)
    double A1 = 0, A2 = 0, A3 = 0;
    if (ok && D.ldim == 1 && D.n_lm > 0) {                 // the landmark sums of k_ba_backsub (uniform branch: ok is thread 0's, see below)
        for (int i = tid; i < D.bs_blocks; i += nt) { A1 += D.part[i]; A2 += D.part[BA_PART_MAX + i]; A3 += D.part[2 * BA_PART_MAX + i]; }
    }
    __syncthreads();
    block_reduce3<false>(A1, A2, A3, s_part);
    if (tid == 0) {
        BACtl cl = *ctl;
        if (D.ldim == 1 && D.n_lm > 0) { cl.acc1 += A1; cl.acc2 += A2; cl.acc3 += A3; }
        s_flag = d_ctl_candidate(cl, O, ok, P1, P2);
        *D.ctl = cl;
    }
    __syncthreads();
    if (!s_flag) return;
    // candidate = Plus(x, step .* scale), step = -y
    for (int k = tid; k < D.n_kf; k += nt) {
        const int pc = D.pose_col[k];
        double out[7];
        if (pc >= 0) {
            double d[6];
            for (int c = 0; c < 6; c++) d[c] = -D.yf[pc + c] * D.scale_f[pc + c];
            d_se3_left_plus(D.x_pose + 7 * k, d, out);
        } else for (int c = 0; c < 7; c++) out[c] = D.x_pose[7 * k + c];
        for (int c = 0; c < 7; c++) D.c_pose[7 * k + c] = out[c];
        d_pose_to_RT(out, D.c_RT + 12 * k);
    }
    if (D.ldim != 1) {                                      // (inverse-depth form: k_ba_backsub wrote the candidates)
        double *__restrict__ c_lam = D.c_lam; const double *__restrict__ x_lam = D.x_lam, *__restrict__ yl = D.yl, *__restrict__ scale_l = D.scale_l;
#pragma unroll 4
        for (int l = tid; l < D.n_lm * D.ldim; l += nt) c_lam[l] = x_lam[l] - yl[l] * scale_l[l];
    }
}
__global__ __launch_bounds__(1024) void k_ba_candidate(BADev D, BAOpt O) { b_ba_candidate(D, O); }
__global__ __launch_bounds__(1024) void k_ba_candidate_B(const BADev *__restrict__ arr, BAOpt O) { const BADev &D = arr[blockIdx.z]; b_ba_candidate(D, O); }

// ---------------------------------------------------------------------------------- decision (1 block)
__device__ __forceinline__ void b_ba_decide(const BADev &D, BAOpt O, int seq)
{
    BACtl *ctl = D.ctl;
    // The host's look-ahead control (ba_run): the outcome of iteration seq goes into pinned host memory on every way out of this
    // kernel -- one store instead of a 4-byte hipMemcpyAsync + event in the stream (~10 us of stream time each in rounds 2-3).
    if (ctl->done || !ctl->step_valid) {
        if (seq >= 0 && threadIdx.x == 0) { *(volatile int *)D.flag_h = 2 * seq + (ctl->done ? 1 : 0); __threadfence_system(); }
        return;
    }
    __shared__ double s_part[3][16];
    __shared__ int s_accept;
    const int tid = threadIdx.x, nt = blockDim.x;
    // |x - candidate|^2 and |candidate|^2 over the variable blocks
    double sn = 0, xn = 0;
    for (int k = tid; k < D.n_kf; k += nt) {
        if (D.pose_col[k] < 0) continue;
        for (int c = 0; c < 7; c++) {
            const double d = D.x_pose[7 * k + c] - D.c_pose[7 * k + c];
            sn += d * d; xn += D.c_pose[7 * k + c] * D.c_pose[7 * k + c];
        }
    }
    double cpart = 0;
    if (D.ldim == 1) {                                      // (per work-group sums of k_ba_backsub and k_ba_cost)
        if (D.n_lm > 0) for (int i = tid; i < D.bs_blocks; i += nt) { sn += D.part[3 * BA_PART_MAX + i]; xn += D.part[4 * BA_PART_MAX + i]; }
        for (int i = tid; i < D.cost_blocks; i += nt) cpart += D.part[5 * BA_PART_MAX + i];
    }
    else {
#pragma unroll 4
        for (int l = tid; l < D.n_lm * D.ldim; l += nt) {
            const int lm = l / 3;
            if (!d_lm_has(D, lm)) continue;
            const double d = D.x_lam[l] - D.c_lam[l];
            sn += d * d; xn += D.c_lam[l] * D.c_lam[l];
        }
    }
    double SN = sn, XN = xn, z = cpart;
    block_reduce3<false>(SN, XN, z, s_part);
    if (tid == 0) {
        BACtl cl = *ctl;
        cl.cost_acc += z;
        s_accept = d_ctl_decide(cl, O, SN, XN);
        *D.ctl = cl;
        if (seq >= 0) { *(volatile int *)D.flag_h = 2 * seq + (cl.done ? 1 : 0); __threadfence_system(); }
    }
    __syncthreads();
    if (!s_accept) return;
    // x <- candidate ; clear the pose-side accumulators for the re-linearisation
    for (int e = tid; e < 7 * D.n_kf; e += nt) D.x_pose[e] = D.c_pose[e];
    for (int e = tid; e < 12 * D.n_kf; e += nt) D.x_RT[e] = D.c_RT[e];
    {
        double *__restrict__ x_lam = D.x_lam; const double *__restrict__ c_lam = D.c_lam;
#pragma unroll 8
        for (int l = tid; l < D.n_lm * D.ldim; l += nt) x_lam[l] = c_lam[l];
    }
    if (D.big) return;                                      // k_ba_zero_lin
    {   // 32-byte stores: this one work-group clears H on the iteration's critical path -- the 32 x 32 tiles on and right of the diagonal
        // only (H is its upper triangle: 450 of the 820 KB for 50 keyframes), a row per wavefront
        typedef double d4 __attribute__((ext_vector_type(4)));
        const d4 z = {0., 0., 0., 0.};                      // (nfp is a multiple of 32, the pool is 256-byte aligned)
        for (int r = tid >> 6; r < D.nfp; r += nt >> 6) {
            d4 *row = (d4 *)(D.H + (long long)r * D.nfp);
            for (int c4 = (r & ~31) / 4 + (tid & 63); c4 < D.nfp / 4; c4 += 64) row[c4] = z;
        }
    }
    for (int e = tid; e < D.nfp; e += nt) D.bf[e] = 0;
}
__global__ __launch_bounds__(1024) void k_ba_decide(BADev D, BAOpt O, int seq) { b_ba_decide(D, O, seq); }
__global__ __launch_bounds__(1024) void k_ba_decide_B(const BADev *__restrict__ arr, BAOpt O, int seq) { const BADev &D = arr[blockIdx.z]; b_ba_decide(D, O, seq); }

// ================================================================================== 3-D point landmarks (ldim = 3)
// Optimizer::localBA / looseBA / fullBA with buse_inv_depth: 0 (src/optimizer.cpp:207-209, :333-384): every observation is
// a {pose, X} residual block, no anchors.  Same trust-region loop, same reduced system, same Cholesky; what changes is
// the e-block: 3x3 instead of a scalar.  Per iteration
//   k_ba_linearize_xyz : wavefront per point, lane per residual block: E^T E (6), E^T b (3), three rows of W = E^T F,
//                        observer blocks of H / F^T b pre-aggregated in LDS
//   k_ba_iter_begin    : (shared) bookkeeping + clamped LM diagonal
//   k_ba_xyz_prep      : per point M = S E^T E S + D^2, M^-1 (Cholesky), C = S M^-1 S = L_c L_c^T, Wp rows = L_c^T W,
//                        ep = L_c^T E^T b  ->  W^T C W = Wp^T Wp and W^T C E^T b = Wp^T ep: k_ba_schur_gemm runs unchanged
//   k_ba_backsub_xyz   : y_l = M^-1 S (E^T b - W_l (s . y_f)) and the landmark part of the model cost change
//   k_ba_cost_xyz      : robustified cost at the candidate + the N4 outputs
// dynamic LDS of the lineariser: 4 * 3 * nfp (W rows per wavefront) + n_opt * 27 doubles
__global__ __launch_bounds__(256) void k_ba_linearize_xyz(BADev D)
{
    BACtl *ctl = D.ctl;
    if (ctl->done || !ctl->need_lin) return;
    extern __shared__ __align__(16) unsigned char smem_raw[];
    const int n_opt = D.nf / 6;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, nw = blockDim.x >> 6;
    double *wrow = (double *)smem_raw + wave * 3 * D.nfp;
    double *Hoo = (double *)smem_raw + nw * 3 * D.nfp;
    double *bo = Hoo + n_opt * 21;
    for (int e = threadIdx.x; e < n_opt * 27; e += blockDim.x) Hoo[e] = 0;
    __syncthreads();
    const int total_waves = gridDim.x * nw, gw = blockIdx.x * nw + wave;
    const int chunk = (D.n_lm + total_waves - 1) / total_waves;
    const int i0 = gw * chunk, i1 = min(D.n_lm, i0 + chunk);
    double cost = 0;
    for (int pt = i0; pt < i1; pt++) {
        const int beg = D.lm_ptr[pt], end = D.lm_ptr[pt + 1];
        const double X[3] = {D.x_lam[3 * pt], D.x_lam[3 * pt + 1], D.x_lam[3 * pt + 2]};
        for (int c = lane; c < 3 * D.nfp; c += 64) wrow[c] = 0;
        wave_lds_sync();
        double ee[6] = {0, 0, 0, 0, 0, 0}, eb[3] = {0, 0, 0};
        for (int base = beg; base < end; base += 64) {
            const int k = base + lane;
            if (k < end) {
                const int type = D.res_type[k], o = D.res_kf[k], co = D.pose_col[o];
                const double uv[2] = {D.res_uv[2 * k], D.res_uv[2 * k + 1]};
                double r[2], Jp[12], Jx[6];
                const int dp = d_residual_xyz<true>(D, type, D.x_RT + 12 * o, X, uv, D.res_sigma[k], r, Jp, Jx);
                const double s = r[0] * r[0] + r[1] * r[1];
                const int orig = D.res_orig[k];
                D.chi2[orig] = s; D.dpos[orig] = (uint8_t)dp;
                double rho0, rho1;
                d_huber(D.huber, s, rho0, rho1);
                cost += 0.5 * rho0;
                const double sc = sqrt(rho1);                 // corrector.cc: rho'' <= 0 -> scale by sqrt(rho')
                r[0] *= sc; r[1] *= sc;
                for (int q = 0; q < 12; q++) Jp[q] *= sc;
                for (int q = 0; q < 6; q++) Jx[q] *= sc;
                ee[0] += Jx[0] * Jx[0] + Jx[3] * Jx[3]; ee[1] += Jx[0] * Jx[1] + Jx[3] * Jx[4]; ee[2] += Jx[0] * Jx[2] + Jx[3] * Jx[5];
                ee[3] += Jx[1] * Jx[1] + Jx[4] * Jx[4]; ee[4] += Jx[1] * Jx[2] + Jx[4] * Jx[5]; ee[5] += Jx[2] * Jx[2] + Jx[5] * Jx[5];
                for (int a = 0; a < 3; a++) eb[a] += Jx[a] * r[0] + Jx[3 + a] * r[1];
                if (co >= 0) {
                    const int ob = co / 6;
                    int t = 0;
                    for (int c = 0; c < 6; c++) {
                        for (int a = 0; a < 3; a++) atomicAdd(&wrow[a * D.nfp + co + c], Jx[a] * Jp[c] + Jx[3 + a] * Jp[6 + c]);
                        atomicAdd(&bo[ob * 6 + c], Jp[c] * r[0] + Jp[6 + c] * r[1]);
                        for (int d = c; d < 6; d++) atomicAdd(&Hoo[ob * 21 + t++], Jp[c] * Jp[d] + Jp[6 + c] * Jp[6 + d]);
                    }
                }
            }
        }
#pragma unroll
        for (int q = 0; q < 6; q++) ee[q] = wave_sum(ee[q]);
#pragma unroll
        for (int a = 0; a < 3; a++) eb[a] = wave_sum(eb[a]);
        if (lane < 6) D.ete6[6 * pt + lane] = ee[lane];
        if (lane < 3) D.etb[3 * pt + lane] = eb[lane];
        wave_lds_sync();
        double *Wg = D.W + (long long)3 * pt * D.nfp;
        for (int c = lane; c < 3 * D.nfp; c += 64) Wg[c] = wrow[c];
        wave_lds_sync();
    }
    __syncthreads();
    for (int e = threadIdx.x; e < n_opt * 21; e += blockDim.x) {
        const double v = Hoo[e];
        if (v != 0.0) {
            const int ob = e / 21;
            int t = e - ob * 21, c = 0, d = 0;
            for (c = 0; c < 6; c++) { if (t < 6 - c) { d = c + t; break; } t -= 6 - c; }
            atomicAdd(&D.H[(long long)(ob * 6 + c) * D.nfp + ob * 6 + d], v);
        }
    }
    for (int e = threadIdx.x; e < n_opt * 6; e += blockDim.x) { const double v = bo[e]; if (v != 0.0) atomicAdd(&D.bf[e], v); }
    __shared__ double s_part[4];
    cost = block_sum(cost, s_part);
    if (threadIdx.x == 0 && cost != 0.0) atomicAdd(&ctl->cost_acc, cost);
}

// lower Cholesky factor of the symmetric 3x3 (a0 a1 a2; . a3 a4; . . a5); returns false if not positive definite
__device__ __forceinline__ bool d_chol3(const double a[6], double L[6])      // L: (l00, l10, l11, l20, l21, l22)
{
    if (!(a[0] > 0.0)) return false;
    L[0] = sqrt(a[0]);
    L[1] = a[1] / L[0];
    const double d1 = a[3] - L[1] * L[1];
    if (!(d1 > 0.0)) return false;
    L[2] = sqrt(d1);
    L[3] = a[2] / L[0];
    L[4] = (a[4] - L[3] * L[1]) / L[2];
    const double d2 = a[5] - L[3] * L[3] - L[4] * L[4];
    if (!(d2 > 0.0)) return false;
    L[5] = sqrt(d2);
    return true;
}

// one wavefront per point (see the block comment above)
__global__ __launch_bounds__(256) void k_ba_xyz_prep(BADev D)
{
    BACtl *ctl = D.ctl;
    if (ctl->done) return;
    const int lane = threadIdx.x & 63;
    const double radius = ctl->radius;
    for (int pt = blockIdx.x * 4 + (threadIdx.x >> 6); pt < D.n_lm; pt += gridDim.x * 4) {
        double *wp = D.Wp + (long long)3 * pt * D.nfp;
        if (D.lm_ptr[pt] == D.lm_ptr[pt + 1]) {                       // a point without residual blocks is not part of the program
            for (int c = lane; c < 3 * D.nfp; c += 64) wp[c] = 0;
            if (lane < 3) D.ep[3 * pt + lane] = 0;
            if (lane < 6) D.minv6[6 * pt + lane] = 0;
            continue;
        }
        const double s0 = D.scale_l[3 * pt], s1 = D.scale_l[3 * pt + 1], s2 = D.scale_l[3 * pt + 2];
        const double *e = D.ete6 + 6 * pt;
        const double M[6] = {s0 * s0 * e[0] + D.diag_l[3 * pt] / radius, s0 * s1 * e[1], s0 * s2 * e[2],
                             s1 * s1 * e[3] + D.diag_l[3 * pt + 1] / radius, s1 * s2 * e[4], s2 * s2 * e[5] + D.diag_l[3 * pt + 2] / radius};
        double L[6];
        bool ok = d_chol3(M, L);
        // M^-1 = L^-T L^-1 ; Li = L^-1 (lower)
        double mi[6] = {0, 0, 0, 0, 0, 0}, Lc[6] = {0, 0, 0, 0, 0, 0};
        if (ok) {
            const double i00 = 1.0 / L[0], i11 = 1.0 / L[2], i22 = 1.0 / L[5];
            const double i10 = -L[1] * i00 * i11, i21 = -L[4] * i11 * i22, i20 = -(L[3] * i00 + L[4] * i10) * i22;
            mi[0] = i00 * i00 + i10 * i10 + i20 * i20; mi[1] = i10 * i11 + i20 * i21; mi[2] = i20 * i22;
            mi[3] = i11 * i11 + i21 * i21; mi[4] = i21 * i22; mi[5] = i22 * i22;
            const double C[6] = {s0 * s0 * mi[0], s0 * s1 * mi[1], s0 * s2 * mi[2], s1 * s1 * mi[3], s1 * s2 * mi[4], s2 * s2 * mi[5]};
            ok = d_chol3(C, Lc);
        }
        if (!ok) { if (lane == 0) ctl->lin_fail = 1; for (int q = 0; q < 6; q++) { mi[q] = 0; Lc[q] = 0; } }
        if (lane < 6) D.minv6[6 * pt + lane] = mi[lane];
        // ep = L_c^T E^T b ; Wp rows r = sum_a L_c[a][r] W[a]
        const double b0 = D.etb[3 * pt], b1 = D.etb[3 * pt + 1], b2 = D.etb[3 * pt + 2];
        if (lane == 0) { D.ep[3 * pt] = Lc[0] * b0 + Lc[1] * b1 + Lc[3] * b2; D.ep[3 * pt + 1] = Lc[2] * b1 + Lc[4] * b2; D.ep[3 * pt + 2] = Lc[5] * b2; }
        const double *w = D.W + (long long)3 * pt * D.nfp;
        for (int c = lane; c < D.nfp; c += 64) {
            const double w0 = w[c], w1 = w[D.nfp + c], w2 = w[2 * D.nfp + c];
            wp[c] = Lc[0] * w0 + Lc[1] * w1 + Lc[3] * w2;
            wp[D.nfp + c] = Lc[2] * w1 + Lc[4] * w2;
            wp[2 * D.nfp + c] = Lc[5] * w2;
        }
    }
}

// one wavefront per point: t = W_l (s . y_f) (3 dot products), y_l = M^-1 S (E^T b - t)
__global__ __launch_bounds__(256) void k_ba_backsub_xyz(BADev D)
{
    BACtl *ctl = D.ctl;
    if (ctl->done) return;
    // G = W^T C W was consumed by k_ba_assemble: clear it for the next iteration's Schur kernels here (many work-groups) instead
    // of a memset launch per iteration
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < (long long)D.nfp * D.nfp; e += (long long)gridDim.x * blockDim.x) D.G[e] = 0;
    if (ctl->lin_fail) return;
    extern __shared__ __align__(16) unsigned char smem_raw[];
    double *sy = (double *)smem_raw;                        // s_j * yf_j
    for (int c = threadIdx.x; c < D.nfp; c += blockDim.x) sy[c] = c < D.nf ? D.scale_f[c] * D.yf[c] : 0.0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    double a1 = 0, a2 = 0, a3 = 0;
    for (int pt = blockIdx.x * 4 + (threadIdx.x >> 6); pt < D.n_lm; pt += gridDim.x * 4) {
        if (D.lm_ptr[pt] == D.lm_ptr[pt + 1]) { if (lane < 3) D.yl[3 * pt + lane] = 0; continue; }
        const double *w = D.W + (long long)3 * pt * D.nfp;
        double t0 = 0, t1 = 0, t2 = 0;
        for (int c = lane; c < D.nfp; c += 64) { const double v = sy[c]; t0 += w[c] * v; t1 += w[D.nfp + c] * v; t2 += w[2 * D.nfp + c] * v; }
        t0 = wave_sum(t0); t1 = wave_sum(t1); t2 = wave_sum(t2);
        if (lane == 0) {
            const double s[3] = {D.scale_l[3 * pt], D.scale_l[3 * pt + 1], D.scale_l[3 * pt + 2]};
            const double b[3] = {D.etb[3 * pt], D.etb[3 * pt + 1], D.etb[3 * pt + 2]}, t[3] = {t0, t1, t2};
            const double *mi = D.minv6 + 6 * pt, *e = D.ete6 + 6 * pt;
            const double u[3] = {s[0] * (b[0] - t[0]), s[1] * (b[1] - t[1]), s[2] * (b[2] - t[2])};
            const double y[3] = {mi[0] * u[0] + mi[1] * u[1] + mi[2] * u[2], mi[1] * u[0] + mi[3] * u[1] + mi[4] * u[2],
                                 mi[2] * u[0] + mi[4] * u[1] + mi[5] * u[2]};
            D.yl[3 * pt] = y[0]; D.yl[3 * pt + 1] = y[1]; D.yl[3 * pt + 2] = y[2];
            const double z[3] = {s[0] * y[0], s[1] * y[1], s[2] * y[2]};                  // S y
            a1 += z[0] * b[0] + z[1] * b[1] + z[2] * b[2];
            a2 += 2.0 * (z[0] * t[0] + z[1] * t[1] + z[2] * t[2])
                + z[0] * (e[0] * z[0] + e[1] * z[1] + e[2] * z[2]) + z[1] * (e[1] * z[0] + e[3] * z[1] + e[4] * z[2]) + z[2] * (e[2] * z[0] + e[4] * z[1] + e[5] * z[2]);
            const double q[3] = {s[0] * t[0], s[1] * t[1], s[2] * t[2]};                  // t^T C t, C = S M^-1 S
            a3 += q[0] * (mi[0] * q[0] + mi[1] * q[1] + mi[2] * q[2]) + q[1] * (mi[1] * q[0] + mi[3] * q[1] + mi[4] * q[2]) + q[2] * (mi[2] * q[0] + mi[4] * q[1] + mi[5] * q[2]);
        }
    }
    __shared__ double s_part[4];
    a1 = block_sum(a1, s_part); a2 = block_sum(a2, s_part); a3 = block_sum(a3, s_part);
    if (threadIdx.x == 0) {
        if (a1 != 0.0) atomicAdd(&ctl->acc1, a1);
        if (a2 != 0.0) atomicAdd(&ctl->acc2, a2);
        if (a3 != 0.0) atomicAdd(&ctl->acc3, a3);
    }
}

__global__ __launch_bounds__(256) void k_ba_cost_xyz(BADev D)
{
    BACtl *ctl = D.ctl;
    if (ctl->done || !ctl->step_valid) return;
    const int lane = threadIdx.x & 63;
    double cost = 0;
    for (int pt = blockIdx.x * 4 + (threadIdx.x >> 6); pt < D.n_lm; pt += gridDim.x * 4) {
        const int beg = D.lm_ptr[pt], end = D.lm_ptr[pt + 1];
        const double X[3] = {D.c_lam[3 * pt], D.c_lam[3 * pt + 1], D.c_lam[3 * pt + 2]};
        for (int k = beg + lane; k < end; k += 64) {
            const double uv[2] = {D.res_uv[2 * k], D.res_uv[2 * k + 1]};
            double r[2];
            const int dp = d_residual_xyz<false>(D, D.res_type[k], D.c_RT + 12 * D.res_kf[k], X, uv, D.res_sigma[k], r, nullptr, nullptr);
            const double s = r[0] * r[0] + r[1] * r[1];
            const int orig = D.res_orig[k];
            D.chi2[orig] = s; D.dpos[orig] = (uint8_t)dp;
            double rho0, rho1;
            d_huber(D.huber, s, rho0, rho1);
            cost += 0.5 * rho0;
        }
    }
    __shared__ double s_part[4];
    cost = block_sum(cost, s_part);
    if (threadIdx.x == 0 && cost != 0.0) atomicAdd(&ctl->cost_acc, cost);
}

// cached R | t of every pose; scales = 1 (Jacobi scaling, when on, overwrites them at the first k_ba_iter_begin)
__device__ __forceinline__ void b_ba_init(const BADev &D)
{
    const long long i0 = (long long)blockIdx.x * blockDim.x + threadIdx.x, stride = (long long)gridDim.x * blockDim.x;
    for (long long k = i0; k < D.n_kf; k += stride) d_pose_to_RT(D.x_pose + 7 * k, D.x_RT + 12 * k);
    for (long long c = i0; c < D.nfp; c += stride) D.scale_f[c] = 1.0;
    const long long NL = (long long)D.n_lm * D.ldim;
    for (long long l = i0; l < NL; l += stride) { D.scale_l[l] = 1.0; if (D.ldim == 3) D.ones[l] = 1.0; }
}
__global__ __launch_bounds__(256) void k_ba_init(BADev D) { b_ba_init(D); }
__global__ __launch_bounds__(256) void k_ba_init_B(const BADev *__restrict__ arr) { const BADev &D = arr[blockIdx.z]; b_ba_init(D); }

// ---------------------------------------------------------------------------------- host
// ---------------------------------------------------------------------------------- resident two-pass localBA
// Optimizer::localBA between its two ceres::Solve calls (src/optimizer.cpp:492-594) and after the second (:637-735), on the
// device: a residual block still in the problem is an outlier when its cached chi2err_ (the value of the LAST Evaluate, N4)
// exceeds the threshold or its depth was not positive; with `deactivate` it is removed from the problem.
// cnt[0] = outliers found by this call, cnt[1] / cnt[2] = a left / right-camera block remains in the problem (:606-608).
__device__ __forceinline__ void b_ba_mark_outliers(const BADev &D, double th, int deactivate, uint8_t *__restrict__ snapshot)
{
    int nbad = 0, left = 0, right = 0;
    for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < D.n_act; k += gridDim.x * blockDim.x) {
        if (D.res_off[k]) continue;
        const int orig = D.res_orig[k];
        const bool bad = D.chi2[orig] > th || D.dpos[orig] == 0;
        if (bad) {
            D.bad_obs[orig] = 1;
            if (snapshot) snapshot[orig] = 1;
            if (deactivate) D.res_off[k] = 1;
            nbad++;
        } else {
            const int type = D.res_type[k];
            left |= type == OV2_RES_LEFT; right |= type == OV2_RES_RIGHT;
        }
    }
    __shared__ int s_cnt[3];
    if (threadIdx.x < 3) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    if (nbad) atomicAdd(&s_cnt[0], nbad);
    if (left) atomicOr(&s_cnt[1], 1);
    if (right) atomicOr(&s_cnt[2], 1);
    __syncthreads();
    if (threadIdx.x == 0) {
        if (s_cnt[0]) atomicAdd(&D.lba_cnt[0], s_cnt[0]);
        if (s_cnt[1]) atomicOr(&D.lba_cnt[1], 1);
        if (s_cnt[2]) atomicOr(&D.lba_cnt[2], 1);
    }
}
__global__ __launch_bounds__(256) void k_ba_mark_outliers(BADev D, double th, int deactivate, uint8_t *__restrict__ snapshot) { b_ba_mark_outliers(D, th, deactivate, snapshot); }
__global__ __launch_bounds__(256) void k_ba_mark_outliers_B(const BADev *__restrict__ arr, double th, int deactivate, uint8_t *__restrict__ snapshot) { const BADev &D = arr[blockIdx.z]; if (D.skip2) return; b_ba_mark_outliers(D, th, deactivate, snapshot); }

// a landmark whose residual blocks were all removed leaves the program (its inverse depth keeps its value)
__device__ __forceinline__ void b_ba_lm_live(const BADev &D)
{
    const int lane = threadIdx.x & 63;
    for (int lm = blockIdx.x * 4 + (threadIdx.x >> 6); lm < D.n_lm; lm += gridDim.x * 4) {
        int live = 0;
        for (int k = D.lm_ptr[lm] + lane; k < D.lm_ptr[lm + 1]; k += 64) live |= !D.res_off[k];
        live = __builtin_amdgcn_ballot_w64(live != 0) != 0;
        if (lane == 0) D.lm_live[lm] = (uint8_t)live;
    }
}
__global__ __launch_bounds__(256) void k_ba_lm_live(BADev D) { b_ba_lm_live(D); }
__global__ __launch_bounds__(256) void k_ba_lm_live_B(const BADev *__restrict__ arr) { const BADev &D = arr[blockIdx.z]; if (D.skip2) return; b_ba_lm_live(D); }

struct ov2_ba_dev {
    BADev D;
    void *pool = nullptr; size_t pool_bytes = 0;
    bool pool_owned = true;             // false: the pool lives in the context's grow-only device scratch (transient small problems)
    int n_res = 0;
    int *lm_order = nullptr;            // landmarks sorted by anchor keyframe (device)
    std::vector<double> h_poses0, h_lam0;
    int device = 0;
};

static size_t al256(size_t v) { return (v + 255) & ~(size_t)255; }
static void ba_destroy(ov2_ba_dev *dev);

// lock-step batch (ov2_local_ba_batch): the problems' pools and staging mirrors are consecutive slices of ONE device / pinned block
struct BASlice { uint8_t *dev_base; size_t dev_cap, dev_used; uint8_t *host_base; size_t host_cap, host_used; std::mutex m; };      // (the problems of a batch are prepared on several host threads)
#define BA_SLICE_FULL (-12345)          // (internal: the caller grows the blocks and starts over)

// persistent host threads of a context (ov2_ctx::ba_host_pool): the problems of a batch are prepared on them (spawning sixteen threads per
// batch was 0.3 ms of its first millisecond), and so are the slices of one large problem's sort (ba_create)
struct BAHostPool {
    std::vector<std::thread> th; std::mutex m; std::condition_variable cv_go, cv_done;
    const std::function<void(int)> *fn = nullptr; int n = 0, gen = 0, busy = 0; std::atomic<int> next{0}; bool quit = false;
    explicit BAHostPool(int nt)
    {
        try { spawn(nt); }
        catch (...) { { std::lock_guard<std::mutex> l(m); quit = true; } cv_go.notify_all(); for (auto &t : th) t.join(); th.clear(); throw; }
    }
    void spawn(int nt)
    {
        for (int t = 0; t < nt; t++)
            th.emplace_back([this] {
                int seen = 0;
                for (;;) {
                    { std::unique_lock<std::mutex> l(m); cv_go.wait(l, [&] { return quit || gen != seen; }); if (quit) return; seen = gen; }
                    for (int i; (i = next.fetch_add(1)) < n;) (*fn)(i);
                    { std::lock_guard<std::mutex> l(m); busy--; }
                    cv_done.notify_one();
                }
            });
    }
    ~BAHostPool() { { std::lock_guard<std::mutex> l(m); quit = true; } cv_go.notify_all(); for (auto &t : th) t.join(); }
    void run(int count, const std::function<void(int)> &f)              // f(0 .. count-1); the caller takes part
    {
        if (th.empty() || count <= 1) { for (int i = 0; i < count; i++) f(i); return; }
        { std::lock_guard<std::mutex> l(m); fn = &f; n = count; next.store(0); busy = (int)th.size(); gen++; }
        cv_go.notify_all();
        for (int i; (i = next.fetch_add(1)) < count;) f(i);
        std::unique_lock<std::mutex> l(m); cv_done.wait(l, [&] { return busy == 0; });
    }
};

static BAHostPool *ba_host_pool_of(ov2_ctx *ctx)
{
    if (!ctx->ba_host_pool) {
        try { ctx->ba_host_pool = new BAHostPool(15); }               // (no threads to be had: the caller works serially)
        catch (...) { ctx->ba_host_pool = nullptr; }
        ctx->ba_host_pool_free = [](void *q) { delete (BAHostPool *)q; };
    }
    return (BAHostPool *)ctx->ba_host_pool;
}

// transient: the problem lives for one ov2_ba_solve call -- small pools then come out of the context's device scratch instead of
// a hipMalloc / hipFree pair (~100 us, more than a whole ceresPnP solve)
static int ba_create(ov2_ctx *ctx, const ov2_ba_problem *p, ov2_ba_dev **out, bool transient = false, BASlice *ext = nullptr)
{
    OV2_REQUIRE(p && out, OV2_EINVAL, "NULL problem");
    OV2_REQUIRE(p->n_kf > 0 && p->n_lm >= 0 && p->n_res >= 0, OV2_EINVAL, "bad problem sizes");
    OV2_REQUIRE(p->poses && p->kf_const, OV2_EINVAL, "NULL pose arrays");
    OV2_REQUIRE(p->n_lm == 0 || (p->invdepth && p->lm_anchor_kf && p->lm_anchor_uv), OV2_EINVAL, "NULL landmark arrays");
    OV2_REQUIRE(p->n_res == 0 || (p->res_type && p->res_kf && p->res_lm && p->res_uv && p->res_sigma), OV2_EINVAL, "NULL residual arrays");
    // validate + landmark-sorted order of the active residual blocks (a STABLE counting sort: blocks of a landmark keep the
    // caller's order); pose-only blocks (OV2_RES_PNP) go to their own list.  Large problems (a 590 k-block localBA: 3.8 ms of the
    // call were this sort and the staging fill) split the residual range over a few host threads: per-thread counts, offsets
    // = landmark prefix + the counts of the lower-numbered threads, so the result is identical to the serial sort.
    // (a 25-KF window of 69 k blocks: 2 threads; the problems of a batch are prepared side by side already: one thread each)
    int NT = (p->n_res >= (1 << 16) && !ext) ? std::min(8, p->n_res >> 15) : 1;
    BAHostPool *hpool = NT > 1 ? ba_host_pool_of(ctx) : nullptr;
    if (!hpool) NT = 1;
    const bool dbg_laps = ctx->debug != 0 && !ext;
    const auto tc0 = std::chrono::steady_clock::now();
    auto clap = [&](const char *what) {
        if (dbg_laps) fprintf(stderr, "[ov2 ba_create] %-34s %8.3f ms since entry\n", what, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tc0).count());
    };
    std::vector<std::vector<int>> cntT((size_t)NT, std::vector<int>((size_t)p->n_lm + 1, 0));
    std::vector<int> nactT((size_t)NT, 0), npoT((size_t)NT, 0);
    std::vector<const char *> errT((size_t)NT, nullptr);
    auto range_of = [&](int t, int &b, int &e) { b = (int)((long long)p->n_res * t / NT); e = (int)((long long)p->n_res * (t + 1) / NT); };
    auto run_threads = [&](auto &&fn) {
        if (NT == 1) { fn(0); return; }
        const std::function<void(int)> f = fn;                          // (the context's persistent threads: two spawns per call were 0.1 - 0.3 ms)
        hpool->run(NT, f);
    };
    run_threads([&](int t) {
        int b, e; range_of(t, b, e);
        std::vector<int> &cn = cntT[(size_t)t];
        int na_t = 0, np_t = 0;
        const char *err = nullptr;
        for (int i = b; i < e && !err; i++) {
            if (p->res_active && !p->res_active[i]) continue;
            if (p->res_type[i] > OV2_RES_PNP) { err = "unknown residual type"; break; }
            if (!(p->res_sigma[i] > 0)) { err = "res_sigma must be positive"; break; }
            if (p->res_type[i] == OV2_RES_PNP) {
                if (!p->res_xyz) { err = "OV2_RES_PNP blocks need res_xyz"; break; }
                if (p->res_kf[i] < 0 || p->res_kf[i] >= p->n_kf) { err = "res_kf out of range"; break; }
                np_t++;
                continue;
            }
            const int lm = p->res_lm[i];
            if (lm < 0 || lm >= p->n_lm) { err = "res_lm out of range"; break; }
            if (p->res_type[i] != OV2_RES_RIGHT_ANCH && (p->res_kf[i] < 0 || p->res_kf[i] >= p->n_kf)) { err = "res_kf out of range"; break; }
            // The observer of a LEFT / RIGHT block is never the landmark's anchor keyframe (the reference skips the anchor's own
            // mono observation, src/optimizer.cpp:290-296, and gives its right-camera observation the RIGHT_ANCH factor): the lineariser
            // relies on it (J_observer = -J_anchor serves both the observer's diagonal block and the anchor-observer block)
            if (p->res_type[i] != OV2_RES_RIGHT_ANCH && p->res_kf[i] == p->lm_anchor_kf[lm]) { err = "a LEFT / RIGHT block observes its landmark from the anchor keyframe (use OV2_RES_RIGHT_ANCH)"; break; }
            cn[lm]++; na_t++;
        }
        nactT[(size_t)t] = na_t; npoT[(size_t)t] = np_t; errT[(size_t)t] = err;
    });
    for (int t = 0; t < NT; t++) OV2_REQUIRE(errT[(size_t)t] == nullptr, OV2_EINVAL, errT[(size_t)t]);
    clap("validate + count");
    std::vector<int> cnt(p->n_lm + 1, 0);                              // cnt[l] = first sorted index of landmark l (CSR)
    int n_act = 0, n_po = 0;
    for (int t = 0; t < NT; t++) { n_act += nactT[(size_t)t]; n_po += npoT[(size_t)t]; }
    {
        int run = 0;
        for (int l = 0; l < p->n_lm; l++) {
            OV2_REQUIRE(p->lm_anchor_kf[l] >= 0 && p->lm_anchor_kf[l] < p->n_kf, OV2_EINVAL, "lm_anchor_kf out of range");
            cnt[l] = run;
            for (int t = 0; t < NT; t++) { const int c = cntT[(size_t)t][l]; cntT[(size_t)t][l] = run; run += c; }   // cntT becomes the thread's fill cursor
        }
        cnt[p->n_lm] = run;
    }
    std::vector<int> pose_col(p->n_kf);
    int n_opt = 0;
    for (int k = 0; k < p->n_kf; k++) pose_col[k] = p->kf_const[k] ? -1 : 6 * n_opt++;
    const int nf = 6 * n_opt, nfp = std::max(BA_TILE, (nf + BA_TILE - 1) / BA_TILE * BA_TILE);
    OV2_REQUIRE(nfp <= BA_MAX_NFP, OV2_EUNSUPPORTED, "more than 1024 optimised keyframes: dense reduced system too large");
    // the per-residual upload arrays are filled straight into the context's PINNED host scratch: the H2D copies below are then
    // real asynchronous DMA (from pageable std::vectors every copy went through the runtime's staging buffer, ~2.5 ms for the
    // 20 MB of a 590 k-block problem) and no 20 MB of vectors is allocated and zeroed per call
    int *res_kf, *res_orig, *po_kf, *po_orig;
    uint8_t *res_type;
    double *res_uv, *res_sigma, *po_xyz, *po_uv, *po_sigma;
    // Round 3: the staging buffer MIRRORS the first eleven arrays of the device pool (same offsets), so that everything a solve
    // needs from the host goes up in ONE copy instead of eleven (each ~15 us of launch overhead: a third of ba_create on a
    // 69 k-block window)
    const size_t nl = (size_t)std::max(1, p->n_lm), na = (size_t)std::max(1, n_act), nr = (size_t)std::max(1, p->n_res);
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off += al256(bytes); return o; };
    const size_t o_pose_col = take(4 * (size_t)p->n_kf), o_lm_ptr = take(4 * (nl + 1)), o_lm_anchor = take(4 * nl), o_lm_auv = take(16 * nl);
    const size_t o_res_type = take(na), o_res_kf = take(4 * na), o_res_orig = take(4 * na), o_res_uv = take(16 * na), o_res_sigma = take(8 * na);
    const size_t o_lm_order = take(4 * nl), o_lm_live = take(nl);
    const size_t o_pose0 = take(56 * (size_t)p->n_kf), o_lam0 = take(8 * nl);      // initial parameters (the batch's reset kernel copies them on the device)
    const size_t up_bytes = off;                                       // [0, up_bytes) of the pool = the staging buffer
    uint8_t *hs = nullptr;
    {
        const size_t np_h = (size_t)std::max(1, n_po);
        size_t hoff = up_bytes;
        auto htake = [&](size_t bytes) { const size_t o = hoff; hoff += (bytes + 255) & ~(size_t)255; return o; };
        const size_t h6 = htake(4 * np_h), h7 = htake(4 * np_h), h8 = htake(24 * np_h), h9 = htake(16 * np_h), h10 = htake(8 * np_h);
        if (ext) {
            std::lock_guard<std::mutex> l(ext->m);
            if (ext->host_used + hoff > ext->host_cap) { ext->host_used += al256(hoff); return BA_SLICE_FULL; }    // (keeps counting: the caller learns the total)
            hs = ext->host_base + ext->host_used; ext->host_used += al256(hoff);
        } else {
        const int rch = ctx->reserve_host(hoff);
        if (rch != OV2_OK) return rch;
        hs = (uint8_t *)ctx->h_scratch;
        }
        res_kf = (int *)(hs + o_res_kf); res_orig = (int *)(hs + o_res_orig); res_type = hs + o_res_type; res_uv = (double *)(hs + o_res_uv); res_sigma = (double *)(hs + o_res_sigma);
        po_kf = (int *)(hs + h6); po_orig = (int *)(hs + h7); po_xyz = (double *)(hs + h8); po_uv = (double *)(hs + h9); po_sigma = (double *)(hs + h10);
    }
    std::vector<int> poStart((size_t)NT + 1, 0);
    for (int t = 0; t < NT; t++) poStart[(size_t)t + 1] = poStart[(size_t)t] + npoT[(size_t)t];
    run_threads([&](int t) {
        int b, e; range_of(t, b, e);
        std::vector<int> &fill = cntT[(size_t)t];
        int kp = poStart[(size_t)t];
        for (int i = b; i < e; i++) {
            if (p->res_active && !p->res_active[i]) continue;
            if (p->res_type[i] == OV2_RES_PNP) {
                po_kf[kp] = p->res_kf[i]; po_orig[kp] = i; po_sigma[kp] = p->res_sigma[i];
                po_uv[2 * kp] = p->res_uv[2 * i]; po_uv[2 * kp + 1] = p->res_uv[2 * i + 1];
                for (int c = 0; c < 3; c++) po_xyz[3 * kp + c] = p->res_xyz[3 * i + c];
                kp++;
                continue;
            }
            const int k = fill[p->res_lm[i]]++;
            res_type[k] = p->res_type[i]; res_kf[k] = p->res_type[i] == OV2_RES_RIGHT_ANCH ? p->lm_anchor_kf[p->res_lm[i]] : p->res_kf[i];
            res_orig[k] = i; res_uv[2 * k] = p->res_uv[2 * i]; res_uv[2 * k + 1] = p->res_uv[2 * i + 1]; res_sigma[k] = p->res_sigma[i];
        }
    });

    clap("fill staging (sorted blocks)");
    OV2_HIP_CHECK(hipSetDevice(ctx->device));
    ov2_ba_dev *dev = new (std::nothrow) ov2_ba_dev();
    OV2_REQUIRE(dev != nullptr, OV2_ENOMEM, "out of host memory");
    dev->device = ctx->device; dev->n_res = p->n_res;
    if (!ext) dev->h_poses0.assign(p->poses, p->poses + 7 * (size_t)p->n_kf);
    if (!ext) dev->h_lam0.assign(p->invdepth, p->invdepth + (p->n_lm > 0 ? p->n_lm : 0));
    BADev &D = dev->D;
    memset(&D, 0, sizeof(D));
    D.n_kf = p->n_kf; D.n_lm = p->n_lm; D.n_act = n_act; D.nf = nf; D.nfp = nfp; D.n_po = n_po; D.ldim = 1; D.n_res = p->n_res;
    {   // beyond what the LDS-resident lineariser / Cholesky hold (~90 optimised keyframes): sparse W + HBM Cholesky (BADev::big)
        const size_t lin_lds = 8 * (8 * (size_t)nfp + (size_t)n_opt * 27 + 4 * (size_t)n_opt * 21 + 4 * (size_t)LIN_RED) + 64;
        const size_t chol_lds = chol_lds_bytes(nf, nfp);
        D.big = (lin_lds > 159 * 1024 || chol_lds > 150 * 1024 || nf > CH_MAX_LDS_N) ? 1 : 0;
        if (ctx->ba_force_large) D.big = 1;                                    // OV2_OPT_BA_FORCE_LARGE: the path on small problems (tests)
        // beyond ~570 optimised keyframes the big-path linearisers cannot pre-aggregate the observer blocks in LDS either
        D.lin_direct = (D.big && 8 * ((size_t)n_opt * 27 + 4 * (size_t)LIN_RED) + 64 > 159 * 1024) ? 1 : 0;
        if (ctx->ba_lin_direct && D.big) D.lin_direct = 1;                     // OV2_OPT_BA_LIN_DIRECT (tests: force it on small problems)
        D.chol_hbm = D.big; D.lin_waves = 4;
    }
    // big path: the slots of the sparse W (one per landmark and optimised keyframe seeing or anchoring it) and their per-keyframe lists
    std::vector<int> cw_ptr(p->n_lm + 1, 0), cw_col, cw_lm, res_cw, lm_cwa, kfl_ptr(n_opt + 1, 0), kfl_idx;
    if (D.big) {
        res_cw.assign(std::max(1, n_act), -1); lm_cwa.assign(std::max(1, p->n_lm), -1);
        std::vector<int> slot_of(std::max(1, n_opt), -1), touched;
        for (int l = 0; l < p->n_lm; l++) {
            cw_ptr[l] = (int)cw_col.size();
            touched.clear();
            auto get = [&](int col) {
                const int ob = col / 6;
                if (slot_of[ob] < 0) { slot_of[ob] = (int)cw_col.size(); cw_col.push_back(col); cw_lm.push_back(l); touched.push_back(ob); }
                return slot_of[ob];
            };
            if (cnt[l] != cnt[l + 1]) {
                const int ca = pose_col[p->lm_anchor_kf[l]];
                if (ca >= 0) lm_cwa[l] = get(ca);
                for (int k = cnt[l]; k < cnt[l + 1]; k++) {
                    if (res_type[k] == OV2_RES_RIGHT_ANCH) continue;
                    const int co = pose_col[res_kf[k]];
                    if (co >= 0) res_cw[k] = get(co);
                }
            }
            for (int ob : touched) slot_of[ob] = -1;
        }
        cw_ptr[p->n_lm] = (int)cw_col.size();
        for (int c : cw_col) kfl_ptr[c / 6 + 1]++;
        for (int k = 0; k < n_opt; k++) kfl_ptr[k + 1] += kfl_ptr[k];
        kfl_idx.resize(cw_col.size());
        std::vector<int> kfill(kfl_ptr.begin(), kfl_ptr.end() - 1);
        for (size_t j = 0; j < cw_col.size(); j++) kfl_idx[kfill[cw_col[j] / 6]++] = (int)j;
    }
    D.n_cw = (int)cw_col.size();
    const size_t ncw = (size_t)std::max(1, D.n_cw);
    const size_t o_x_pose = take(56 * (size_t)p->n_kf), o_c_pose = take(56 * (size_t)p->n_kf), o_x_RT = take(96 * (size_t)p->n_kf), o_c_RT = take(96 * (size_t)p->n_kf);
    const size_t o_x_lam = take(8 * nl), o_c_lam = take(8 * nl), o_scale_f = take(8 * (size_t)nfp), o_diag_f = take(8 * (size_t)nfp);
    const size_t o_scale_l = take(8 * nl), o_diag_l = take(8 * nl), o_ete = take(8 * nl), o_etb = take(8 * nl), o_cl = take(8 * nl), o_ce = take(8 * nl);
    const size_t o_W = take(D.big ? 256 : 8 * nl * nfp), o_H = take(8 * (size_t)nfp * nfp), o_G = take(8 * (size_t)nfp * nfp), o_S = take(8 * (size_t)nfp * nfp);
    const size_t o_cww = take(48 * ncw), o_cw_ptr = take(4 * (nl + 1)), o_cw_col = take(4 * ncw), o_cw_lm = take(4 * ncw);
    const size_t o_res_cw = take(4 * na), o_lm_cwa = take(4 * nl), o_kfl_ptr = take(4 * ((size_t)n_opt + 1)), o_kfl_idx = take(4 * ncw);
    const size_t o_bf = take(8 * (size_t)nfp), o_v = take(8 * (size_t)nfp), o_yf = take(8 * (size_t)nfp), o_yl = take(8 * nl);
    const size_t o_Linv = take(8 * (size_t)nfp * 32);
    const size_t o_chi2 = take(8 * nr), o_dpos = take(nr), o_ctl = take(sizeof(BACtl));
    const size_t o_res_off = take(na), o_bad_obs = take(nr), o_lba_cnt = take(64), o_part = take(8 * 7 * BA_PART_MAX);
    const size_t npo = (size_t)std::max(1, n_po);
    const size_t o_po_kf = take(4 * npo), o_po_orig = take(4 * npo), o_po_xyz = take(24 * npo), o_po_uv = take(16 * npo), o_po_sigma = take(8 * npo);
    dev->pool_bytes = off;
    if (ext) {
        std::lock_guard<std::mutex> l(ext->m);
        if (ext->dev_used + off > ext->dev_cap) { ext->dev_used += al256(off); delete dev; return BA_SLICE_FULL; }
        dev->pool = ext->dev_base + ext->dev_used; dev->pool_owned = false; ext->dev_used += al256(off);
    } else if (transient && off <= ((size_t)64 << 20)) {               // (the context keeps the largest pool it has seen: grow-only scratch)
        const int rcs = ctx->reserve_device(off);
        if (rcs != OV2_OK) { delete dev; return rcs; }
        dev->pool = ctx->d_scratch; dev->pool_owned = false;
    } else {
        hipError_t e = hipMalloc(&dev->pool, dev->pool_bytes);
        if (e != hipSuccess) { delete dev; ov2_set_error("hipMalloc(%zu): %s", off, hipGetErrorString(e)); return OV2_ENOMEM; }
    }
    uint8_t *b = (uint8_t *)dev->pool;
    D.pose_col = (int *)(b + o_pose_col); D.lm_ptr = (int *)(b + o_lm_ptr); D.lm_anchor = (int *)(b + o_lm_anchor); D.lm_auv = (double *)(b + o_lm_auv);
    D.res_type = b + o_res_type; D.res_kf = (int *)(b + o_res_kf); D.res_orig = (int *)(b + o_res_orig); D.res_uv = (double *)(b + o_res_uv); D.res_sigma = (double *)(b + o_res_sigma);
    D.x_pose = (double *)(b + o_x_pose); D.c_pose = (double *)(b + o_c_pose); D.x_RT = (double *)(b + o_x_RT); D.c_RT = (double *)(b + o_c_RT);
    D.x_lam = (double *)(b + o_x_lam); D.c_lam = (double *)(b + o_c_lam); D.scale_f = (double *)(b + o_scale_f); D.diag_f = (double *)(b + o_diag_f);
    D.scale_l = (double *)(b + o_scale_l); D.diag_l = (double *)(b + o_diag_l); D.ete = (double *)(b + o_ete); D.etb = (double *)(b + o_etb);
    D.part = (double *)(b + o_part);
    D.cl = (double *)(b + o_cl); D.ce = (double *)(b + o_ce); D.W = (double *)(b + o_W); D.H = (double *)(b + o_H); D.G = (double *)(b + o_G); D.S = (double *)(b + o_S);
    D.Linv = (double *)(b + o_Linv);
    D.cww = (double *)(b + o_cww); D.cw_ptr = (int *)(b + o_cw_ptr); D.cw_col = (int *)(b + o_cw_col); D.cw_lm = (int *)(b + o_cw_lm);
    D.res_cw = (int *)(b + o_res_cw); D.lm_cwa = (int *)(b + o_lm_cwa); D.kfl_ptr = (int *)(b + o_kfl_ptr); D.kfl_idx = (int *)(b + o_kfl_idx);
    D.bf = (double *)(b + o_bf); D.v = (double *)(b + o_v); D.yf = (double *)(b + o_yf); D.yl = (double *)(b + o_yl);
    D.chi2 = (double *)(b + o_chi2); D.dpos = b + o_dpos; D.ctl = (BACtl *)(b + o_ctl);
    dev->lm_order = (int *)(b + o_lm_order);
    D.lm_order_b = dev->lm_order; D.pose0 = (const double *)(b + o_pose0); D.lam0 = (const double *)(b + o_lam0);
    D.res_off = b + o_res_off; D.lm_live = b + o_lm_live; D.bad_obs = b + o_bad_obs; D.lba_cnt = (int *)(b + o_lba_cnt);
    D.po_kf = (int *)(b + o_po_kf); D.po_orig = (int *)(b + o_po_orig); D.po_xyz = (double *)(b + o_po_xyz); D.po_uv = (double *)(b + o_po_uv); D.po_sigma = (double *)(b + o_po_sigma);
    for (int i = 0; i < 4; i++) { D.calib_l[i] = p->calib_l[i]; D.calib_r[i] = p->calib_r[i]; }
    {   // Trl: normalised quaternion -> R (host)
        double q[4] = {p->T_rl[3], p->T_rl[4], p->T_rl[5], p->T_rl[6]};
        const double n = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
        if (n > 0) { q[0] /= n; q[1] /= n; q[2] /= n; q[3] /= n; } else { q[0] = q[1] = q[2] = 0; q[3] = 1; }
        const double x = q[0], y = q[1], z = q[2], w = q[3];
        D.Rrl[0] = 1 - 2 * (y * y + z * z); D.Rrl[1] = 2 * (x * y - z * w); D.Rrl[2] = 2 * (x * z + y * w);
        D.Rrl[3] = 2 * (x * y + z * w); D.Rrl[4] = 1 - 2 * (x * x + z * z); D.Rrl[5] = 2 * (y * z - x * w);
        D.Rrl[6] = 2 * (x * z - y * w); D.Rrl[7] = 2 * (y * z + x * w); D.Rrl[8] = 1 - 2 * (x * x + y * y);
        D.trl[0] = p->T_rl[0]; D.trl[1] = p->T_rl[1]; D.trl[2] = p->T_rl[2];
    }
    hipStream_t s = ctx->stream;
#define UP(dst, src, bytes) do { if ((bytes) > 0) { hipError_t _e = hipMemcpyAsync((void *)(dst), (src), (bytes), hipMemcpyHostToDevice, s); \
        if (_e != hipSuccess) { if (dev->pool_owned) (void)hipFree(dev->pool); delete dev; ov2_set_error("H2D: %s", hipGetErrorString(_e)); return OV2_EHIP; } } } while (0)
    {   // the small arrays join the residual arrays in the staging mirror; landmarks are processed anchor by anchor (lm_order)
        int *lm_order = (int *)(hs + o_lm_order);
        {   // stable counting sort by anchor keyframe (a std::stable_sort of 3000 landmarks was 60 us of a 0.45 ms call)
            std::vector<int> first((size_t)p->n_kf + 1, 0);
            for (int l = 0; l < p->n_lm; l++) first[(size_t)p->lm_anchor_kf[l] + 1]++;
            for (int k = 0; k < p->n_kf; k++) first[(size_t)k + 1] += first[(size_t)k];
            for (int l = 0; l < p->n_lm; l++) lm_order[first[(size_t)p->lm_anchor_kf[l]]++] = l;
        }
        uint8_t *lm_live = hs + o_lm_live;
        for (int l = 0; l < p->n_lm; l++) lm_live[l] = cnt[l] != cnt[l + 1];
        memcpy(hs + o_pose_col, pose_col.data(), 4 * (size_t)p->n_kf);
        memcpy(hs + o_lm_ptr, cnt.data(), 4 * ((size_t)p->n_lm + 1));
        if (p->n_lm > 0) { memcpy(hs + o_lm_anchor, p->lm_anchor_kf, 4 * (size_t)p->n_lm); memcpy(hs + o_lm_auv, p->lm_anchor_uv, 16 * (size_t)p->n_lm); }
        memcpy(hs + o_pose0, p->poses, 56 * (size_t)p->n_kf);
        if (p->n_lm > 0) memcpy(hs + o_lam0, p->invdepth, 8 * (size_t)p->n_lm);
    }
    clap("views + small arrays + lm_order");
    UP(b, hs, up_bytes);                                               // ONE copy: pose_col .. lam0
    if (!ext) {                                                        // (batch: k_ba_reset_B clears them)
        hipError_t em = hipMemsetAsync(D.res_off, 0, na, s);
        if (em == hipSuccess) em = hipMemsetAsync(D.bad_obs, 0, nr, s);
        if (em == hipSuccess) em = hipMemsetAsync(D.lba_cnt, 0, 64, s);
        if (em != hipSuccess) { ov2_set_error("hipMemsetAsync: %s", hipGetErrorString(em)); ba_destroy(dev); return OV2_EHIP; }
    }
    UP(D.po_kf, po_kf, 4 * (size_t)n_po); UP(D.po_orig, po_orig, 4 * (size_t)n_po);
    UP(D.po_xyz, po_xyz, 24 * (size_t)n_po); UP(D.po_uv, po_uv, 16 * (size_t)n_po); UP(D.po_sigma, po_sigma, 8 * (size_t)n_po);
    if (D.big) {
        UP(D.cw_ptr, cw_ptr.data(), 4 * ((size_t)p->n_lm + 1)); UP(D.cw_col, cw_col.data(), 4 * (size_t)D.n_cw); UP(D.cw_lm, cw_lm.data(), 4 * (size_t)D.n_cw);
        UP(D.res_cw, res_cw.data(), 4 * (size_t)n_act); UP(D.lm_cwa, lm_cwa.data(), 4 * (size_t)p->n_lm);
        UP(D.kfl_ptr, kfl_ptr.data(), 4 * ((size_t)n_opt + 1)); UP(D.kfl_idx, kfl_idx.data(), 4 * (size_t)D.n_cw);
    }
#undef UP
    // the staging vectors die at return: make sure the copies are done (a batch slice's staging lives until the batch is through)
    if (!ext || D.big) {
        const hipError_t es = hipStreamSynchronize(s);
        if (es != hipSuccess) { ov2_set_error("hipStreamSynchronize: %s", hipGetErrorString(es)); ba_destroy(dev); return OV2_EHIP; }
    }
    clap("upload enqueued + synchronised");
    *out = dev;
    return OV2_OK;
}

// 3-D point landmarks with variable poses (ldim = 3): same device object, point-sorted residual blocks
static int xyzba_create(ov2_ctx *ctx, const ov2_xyzba_problem *p, ov2_ba_dev **out)
{
    OV2_REQUIRE(p && out, OV2_EINVAL, "NULL problem");
    OV2_REQUIRE(p->n_kf > 0 && p->n_pts >= 0 && p->n_res >= 0, OV2_EINVAL, "bad problem sizes");
    OV2_REQUIRE(p->poses, OV2_EINVAL, "NULL pose array");
    OV2_REQUIRE(p->n_pts == 0 || p->xyz, OV2_EINVAL, "NULL point array");
    OV2_REQUIRE(p->n_res == 0 || (p->res_type && p->res_kf && p->res_pt && p->res_uv && p->res_sigma), OV2_EINVAL, "NULL residual arrays");
    std::vector<int> cnt(p->n_pts + 1, 0);
    int n_act = 0;
    for (int i = 0; i < p->n_res; i++) {
        if (p->res_active && !p->res_active[i]) continue;
        OV2_REQUIRE(p->res_type[i] <= OV2_XYZ_RIGHT, OV2_EINVAL, "unknown residual type");
        OV2_REQUIRE(p->res_sigma[i] > 0, OV2_EINVAL, "res_sigma must be positive");
        OV2_REQUIRE(p->res_pt[i] >= 0 && p->res_pt[i] < p->n_pts, OV2_EINVAL, "res_pt out of range");
        OV2_REQUIRE(p->res_kf[i] >= 0 && p->res_kf[i] < p->n_kf, OV2_EINVAL, "res_kf out of range");
        cnt[p->res_pt[i] + 1]++; n_act++;
    }
    for (int l = 0; l < p->n_pts; l++) cnt[l + 1] += cnt[l];
    std::vector<int> pose_col(p->n_kf);
    int n_opt = 0;
    for (int k = 0; k < p->n_kf; k++) pose_col[k] = (p->kf_const && p->kf_const[k]) ? -1 : 6 * n_opt++;
    const int nf = 6 * n_opt, nfp = std::max(BA_TILE, (nf + BA_TILE - 1) / BA_TILE * BA_TILE);
    // Size limits BEFORE anything is allocated or uploaded (W and W' alone are 2 x 24 n_pts nfp bytes).  The 3-D point form keeps
    // W dense: its lineariser holds 3 rows of it per wavefront in LDS next to the observer blocks (4 wavefronts per work-group up
    // to ~200 optimised keyframes, then 2, then 1: ~450), and beyond ~90 keyframes the reduced system is factored by the
    // multi-kernel Cholesky on HBM instead of the one-work-group LDS kernel.
    int lin_waves = 0;
    for (int nw = 4; nw >= 1 && !lin_waves; nw >>= 1)
        if (8 * (3 * (size_t)nw * nfp + (size_t)n_opt * 27) + 64 <= 159 * 1024) lin_waves = nw;
    if (ctx->ba_xyz_lin_waves == 1 || ctx->ba_xyz_lin_waves == 2) lin_waves = lin_waves ? std::min(lin_waves, ctx->ba_xyz_lin_waves) : 0;   // OV2_OPT_BA_XYZ_LIN_WAVES (tests)
    if (!lin_waves || nfp > BA_MAX_NFP) {
        ov2_set_error("too many optimised keyframes (%d) for the 3-D point form (limit ~450: dense W rows in LDS)", n_opt);
        return OV2_EUNSUPPORTED;
    }
    const size_t chol_lds_res = chol_lds_bytes(nf, nfp);
    int chol_hbm = (chol_lds_res > 150 * 1024 || nf > CH_MAX_LDS_N) ? 1 : 0;
    if (ctx->ba_force_large) chol_hbm = 1;                                      // OV2_OPT_BA_FORCE_LARGE (tests: the HBM factorisation on small problems)
    std::vector<int> fill(cnt.begin(), cnt.end() - 1), res_kf(n_act), res_orig(n_act);
    std::vector<uint8_t> res_type(n_act);
    std::vector<double> res_uv(2 * (size_t)n_act), res_sigma(n_act);
    for (int i = 0; i < p->n_res; i++) {
        if (p->res_active && !p->res_active[i]) continue;
        const int k = fill[p->res_pt[i]]++;
        res_type[k] = p->res_type[i]; res_kf[k] = p->res_kf[i]; res_orig[k] = i;
        res_uv[2 * k] = p->res_uv[2 * i]; res_uv[2 * k + 1] = p->res_uv[2 * i + 1]; res_sigma[k] = p->res_sigma[i];
    }
    OV2_HIP_CHECK(hipSetDevice(ctx->device));
    ov2_ba_dev *dev = new (std::nothrow) ov2_ba_dev();
    OV2_REQUIRE(dev != nullptr, OV2_ENOMEM, "out of host memory");
    dev->device = ctx->device; dev->n_res = p->n_res;
    dev->h_poses0.assign(p->poses, p->poses + 7 * (size_t)p->n_kf);
    dev->h_lam0.assign(p->xyz, p->xyz + 3 * (size_t)(p->n_pts > 0 ? p->n_pts : 0));
    BADev &D = dev->D;
    memset(&D, 0, sizeof(D));
    D.n_kf = p->n_kf; D.n_lm = p->n_pts; D.n_act = n_act; D.nf = nf; D.nfp = nfp; D.n_po = 0; D.ldim = 3;
    D.chol_hbm = chol_hbm; D.lin_waves = lin_waves;
    const size_t nl = (size_t)std::max(1, p->n_pts), na = (size_t)std::max(1, n_act), nr = (size_t)std::max(1, p->n_res);
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off += al256(bytes); return o; };
    const size_t o_pose_col = take(4 * (size_t)p->n_kf), o_lm_ptr = take(4 * (nl + 1));
    const size_t o_res_type = take(na), o_res_kf = take(4 * na), o_res_orig = take(4 * na), o_res_uv = take(16 * na), o_res_sigma = take(8 * na);
    const size_t o_x_pose = take(56 * (size_t)p->n_kf), o_c_pose = take(56 * (size_t)p->n_kf), o_x_RT = take(96 * (size_t)p->n_kf), o_c_RT = take(96 * (size_t)p->n_kf);
    const size_t o_x_lam = take(24 * nl), o_c_lam = take(24 * nl), o_scale_f = take(8 * (size_t)nfp), o_diag_f = take(8 * (size_t)nfp);
    const size_t o_scale_l = take(24 * nl), o_diag_l = take(24 * nl), o_etb = take(24 * nl), o_yl = take(24 * nl), o_ep = take(24 * nl), o_ones = take(24 * nl);
    const size_t o_ete6 = take(48 * nl), o_minv6 = take(48 * nl);
    const size_t o_W = take(24 * nl * nfp), o_Wp = take(24 * nl * nfp);
    const size_t o_H = take(8 * (size_t)nfp * nfp), o_G = take(8 * (size_t)nfp * nfp), o_S = take(8 * (size_t)nfp * nfp);
    const size_t o_bf = take(8 * (size_t)nfp), o_v = take(8 * (size_t)nfp), o_yf = take(8 * (size_t)nfp), o_Linv = take(8 * (size_t)nfp * 32);
    const size_t o_chi2 = take(8 * nr), o_dpos = take(nr), o_ctl = take(sizeof(BACtl));
    dev->pool_bytes = off;
    hipError_t e = hipMalloc(&dev->pool, dev->pool_bytes);
    if (e != hipSuccess) { delete dev; ov2_set_error("hipMalloc(%zu): %s", off, hipGetErrorString(e)); return OV2_ENOMEM; }
    uint8_t *b = (uint8_t *)dev->pool;
    D.pose_col = (int *)(b + o_pose_col); D.lm_ptr = (int *)(b + o_lm_ptr);
    D.res_type = b + o_res_type; D.res_kf = (int *)(b + o_res_kf); D.res_orig = (int *)(b + o_res_orig); D.res_uv = (double *)(b + o_res_uv); D.res_sigma = (double *)(b + o_res_sigma);
    D.x_pose = (double *)(b + o_x_pose); D.c_pose = (double *)(b + o_c_pose); D.x_RT = (double *)(b + o_x_RT); D.c_RT = (double *)(b + o_c_RT);
    D.x_lam = (double *)(b + o_x_lam); D.c_lam = (double *)(b + o_c_lam); D.scale_f = (double *)(b + o_scale_f); D.diag_f = (double *)(b + o_diag_f);
    D.scale_l = (double *)(b + o_scale_l); D.diag_l = (double *)(b + o_diag_l); D.etb = (double *)(b + o_etb); D.yl = (double *)(b + o_yl);
    D.ep = (double *)(b + o_ep); D.ones = (double *)(b + o_ones); D.ete6 = (double *)(b + o_ete6); D.minv6 = (double *)(b + o_minv6);
    D.W = (double *)(b + o_W); D.Wp = (double *)(b + o_Wp); D.H = (double *)(b + o_H); D.G = (double *)(b + o_G); D.S = (double *)(b + o_S);
    D.bf = (double *)(b + o_bf); D.v = (double *)(b + o_v); D.yf = (double *)(b + o_yf); D.Linv = (double *)(b + o_Linv);
    D.chi2 = (double *)(b + o_chi2); D.dpos = b + o_dpos; D.ctl = (BACtl *)(b + o_ctl);
    D.cl = D.ones; D.ce = D.ep; D.ete = D.ete6;              // (scalar-landmark views, unused when ldim == 3)
    for (int i = 0; i < 4; i++) { D.calib_l[i] = p->calib_l[i]; D.calib_r[i] = p->calib_r[i]; }
    {
        double q[4] = {p->T_rl[3], p->T_rl[4], p->T_rl[5], p->T_rl[6]};
        const double n = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
        if (n > 0) { q[0] /= n; q[1] /= n; q[2] /= n; q[3] /= n; } else { q[0] = q[1] = q[2] = 0; q[3] = 1; }
        const double x = q[0], y = q[1], z = q[2], w = q[3];
        D.Rrl[0] = 1 - 2 * (y * y + z * z); D.Rrl[1] = 2 * (x * y - z * w); D.Rrl[2] = 2 * (x * z + y * w);
        D.Rrl[3] = 2 * (x * y + z * w); D.Rrl[4] = 1 - 2 * (x * x + z * z); D.Rrl[5] = 2 * (y * z - x * w);
        D.Rrl[6] = 2 * (x * z - y * w); D.Rrl[7] = 2 * (y * z + x * w); D.Rrl[8] = 1 - 2 * (x * x + y * y);
        D.trl[0] = p->T_rl[0]; D.trl[1] = p->T_rl[1]; D.trl[2] = p->T_rl[2];
    }
    hipStream_t s = ctx->stream;
#define UPX(dst, src, bytes) do { if ((bytes) > 0) { hipError_t _e = hipMemcpyAsync((void *)(dst), (src), (bytes), hipMemcpyHostToDevice, s); \
        if (_e != hipSuccess) { (void)hipFree(dev->pool); delete dev; ov2_set_error("H2D: %s", hipGetErrorString(_e)); return OV2_EHIP; } } } while (0)
    UPX(D.pose_col, pose_col.data(), 4 * (size_t)p->n_kf);
    UPX(D.lm_ptr, cnt.data(), 4 * ((size_t)p->n_pts + 1));
    UPX(D.res_type, res_type.data(), (size_t)n_act);
    UPX(D.res_kf, res_kf.data(), 4 * (size_t)n_act);
    UPX(D.res_orig, res_orig.data(), 4 * (size_t)n_act);
    UPX(D.res_uv, res_uv.data(), 16 * (size_t)n_act);
    UPX(D.res_sigma, res_sigma.data(), 8 * (size_t)n_act);
#undef UPX
    {
        const hipError_t es = hipStreamSynchronize(s);
        if (es != hipSuccess) { ov2_set_error("hipStreamSynchronize: %s", hipGetErrorString(es)); ba_destroy(dev); return OV2_EHIP; }
    }
    *out = dev;
    return OV2_OK;
}

static void ba_destroy(ov2_ba_dev *dev)
{
    if (!dev) return;
    (void)hipSetDevice(dev->device);
    if (dev->pool && dev->pool_owned) (void)hipFree(dev->pool);
    delete dev;
}

// state reset of a solve in ONE launch (round 5; single problems: it replaces two pageable H2D copies of the initial parameters, six
// memsets and the upload of the control block -- 60-80 us of host time per pass): x = initial parameters, chi2 = "never evaluated",
// verdicts and removal flags clear (unless keep_state: second pass of localBA), H / G / F^T b / y_f zero, the control block.
// host_chi2: the caller seeds chi2 / depth flags itself (ov2_ba_solve with inactive residual blocks)
__device__ __forceinline__ void b_ba_reset(const BADev &D, const BACtl &ctl0, int keep_state, int host_chi2)
{
    const long long i0 = (long long)blockIdx.x * blockDim.x + threadIdx.x, stride = (long long)gridDim.x * blockDim.x;
    if (i0 == 0) { BACtl c = ctl0; if (keep_state && D.skip2) { c.done = 1; c.need_lin = 0; } *D.ctl = c; }
    if (keep_state && D.skip2) return;
    if (!keep_state) {
        for (long long e = i0; e < 7LL * D.n_kf; e += stride) D.x_pose[e] = D.pose0[e];
        for (long long e = i0; e < D.n_lm; e += stride) D.x_lam[e] = D.lam0[e];
        unsigned long long *chi = (unsigned long long *)D.chi2;
        if (!host_chi2) for (long long e = i0; e < D.n_res; e += stride) { chi[e] = ~0ULL; D.dpos[e] = 0; }          // (NaN pattern: never evaluated)
        for (long long e = i0; e < D.n_res; e += stride) D.bad_obs[e] = 0;
        for (long long e = i0; e < D.n_act; e += stride) D.res_off[e] = 0;
    }
    const long long nn = (long long)D.nfp * D.nfp;
    for (long long e = i0; e < nn; e += stride) { D.H[e] = 0; D.G[e] = 0; }
    for (long long e = i0; e < D.nfp; e += stride) { D.bf[e] = 0; D.yf[e] = 0; }
}
__global__ __launch_bounds__(256) void k_ba_reset(BADev D, BACtl ctl0, int keep_state, int host_chi2) { b_ba_reset(D, ctl0, keep_state, host_chi2); }
__global__ __launch_bounds__(256) void k_ba_reset_B(const BADev *__restrict__ arr, BACtl ctl0, int keep_state) { b_ba_reset(arr[blockIdx.z], ctl0, keep_state, 0); }

// keep_state: continue from the parameters and the cached chi2 / depth flags that are on the device (second pass of
// ov2_local_ba) instead of resetting to the problem's initial values
static int ba_run(ov2_ctx *ctx, ov2_ba_dev *dev, const ov2_ba_options *o, ov2_ba_result *r,
                  const double *chi2_init, const uint8_t *dpos_init, bool keep_state = false)
{
    OV2_REQUIRE(o && r, OV2_EINVAL, "NULL options/result");
    OV2_REQUIRE(o->max_iter >= 0 && o->initial_radius > 0 && o->min_lm_diagonal > 0 && o->min_lm_diagonal <= o->max_lm_diagonal,
                OV2_EINVAL, "bad solver options");
    OV2_HIP_CHECK(hipSetDevice(ctx->device));
    BADev D = dev->D;
    D.huber = o->huber_delta;
    D.min_diag = o->min_lm_diagonal; D.max_diag = o->max_lm_diagonal;
    hipStream_t s = ctx->stream;
    BAOpt O;
    O.max_iter = o->max_iter; O.ftol = o->function_tolerance; O.gtol = o->gradient_tolerance; O.ptol = o->parameter_tolerance;
    O.max_radius = o->max_radius; O.min_radius = o->min_radius; O.min_diag = o->min_lm_diagonal; O.max_diag = o->max_lm_diagonal;
    O.min_rel_decrease = o->min_relative_decrease; O.jacobi = o->jacobi_scaling; O.max_invalid = o->max_consecutive_invalid_steps;

    // size limits first: nothing is created or enqueued for a problem this path cannot solve
    const int n_opt = D.nf / 6;
    const size_t lin_lds = D.big ? 8 * ((D.lin_direct ? 0 : (size_t)(D.nf / 6) * 27) + 4 * (size_t)LIN_RED) + 64
                         : D.ldim == 3 ? 8 * (3 * (size_t)D.lin_waves * D.nfp + (size_t)n_opt * 27) + 64
                                       : 8 * (8 * (size_t)D.nfp + (size_t)n_opt * 27 + 4 * (size_t)n_opt * 21 + 4 * (size_t)LIN_RED) + 64;
    const size_t chol_lds = D.chol_hbm ? 8 * ((size_t)CH_NB * CH_LDP + (size_t)D.nfp) + 64  // k_chol_solve: scratch block + the solution vector
                                  : chol_lds_bytes(D.nf, D.nfp);
    OV2_REQUIRE(lin_lds <= 159 * 1024, OV2_EUNSUPPORTED, "too many optimised keyframes for the LDS-aggregating lineariser");
    OV2_REQUIRE(chol_lds <= 150 * 1024, OV2_EUNSUPPORTED, "reduced system too large for the LDS-panel Cholesky");
    {   // dynamic-LDS limits are per-function, process-wide attributes: raise them once to the hardware maximum (two
        // contexts solving problems of different size on two threads would otherwise race on them)
        static std::once_flag attr_once;
        static hipError_t attr_err = hipSuccess;
        std::call_once(attr_once, [] {
            // the attribute bounds static + dynamic LDS together: leave room for each kernel's __shared__ arrays
            auto raise = [](const void *fn) {
                hipFuncAttributes fa;
                hipError_t e = hipFuncGetAttributes(&fa, fn);
                if (e != hipSuccess) return e;
                for (int kb = 160; kb >= 64; kb -= 32) {             // 160 KB per work-group on gfx950; smaller steps only if refused
                    e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, kb * 1024 - (int)fa.sharedSizeBytes);
                    if (e == hipSuccess) return e;
                    (void)hipGetLastError();
                }
                return e;
            };
            attr_err = raise((const void *)k_ba_linearize<false>);
            if (attr_err == hipSuccess) attr_err = raise((const void *)k_chol_solve);
            if (attr_err == hipSuccess) attr_err = raise((const void *)k_ba_linearize<true>);
            if (attr_err == hipSuccess) attr_err = raise((const void *)k_ba_schur_sparse);
            if (attr_err == hipSuccess) attr_err = raise((const void *)k_ba_linearize_xyz);
            if (attr_err == hipSuccess) attr_err = raise((const void *)k_ba_cholesky);
            if (attr_err == hipSuccess) attr_err = raise((const void *)k_ba_linearize_po);
        });
        OV2_HIP_CHECK(attr_err);
    }
    for (int i = 0; i < 2; i++) if (!ctx->ba_ev[i]) OV2_HIP_CHECK(hipEventCreate(&ctx->ba_ev[i]));      // (the context's: destroyed with it)
    hipEvent_t e0 = ctx->ba_ev[0], e1 = ctx->ba_ev[1];
    // state reset: x = initial parameters, everything else zero, scales one
    const size_t NL = (size_t)D.n_lm * D.ldim;               // per-landmark state entries (1 inverse depth or 3 coordinates each)
    // small inverse-depth problems: one reset kernel instead of the copies / memsets below (b_ba_reset); pose-only fused solves and the
    // other forms keep the round-1 sequence
    const bool fused_po_path = D.n_lm == 0 && D.n_po > 0 && D.nf == 6 && D.ldim == 1 && ctx->ba_pose_only_fused && !(o->max_solver_time_s > 0.0) && !ctx->ba_deterministic;
    const bool one_reset = D.ldim == 1 && !D.big && D.pose0 != nullptr && !fused_po_path;
    if (!keep_state && one_reset) {
        if (chi2_init) OV2_HIP_CHECK(hipMemcpyAsync(D.chi2, chi2_init, 8 * (size_t)dev->n_res, hipMemcpyHostToDevice, s));
        else if (dpos_init) OV2_HIP_CHECK(hipMemsetAsync(D.chi2, 0xFF, 8 * (size_t)std::max(1, dev->n_res), s));
        if (dpos_init) OV2_HIP_CHECK(hipMemcpyAsync(D.dpos, dpos_init, (size_t)dev->n_res, hipMemcpyHostToDevice, s));
        else if (chi2_init) OV2_HIP_CHECK(hipMemsetAsync(D.dpos, 0, (size_t)std::max(1, dev->n_res), s));
    }
    if (!keep_state && !one_reset) {
    OV2_HIP_CHECK(hipMemcpyAsync(D.x_pose, dev->h_poses0.data(), 56 * (size_t)D.n_kf, hipMemcpyHostToDevice, s));
    if (D.n_lm > 0) OV2_HIP_CHECK(hipMemcpyAsync(D.x_lam, dev->h_lam0.data(), 8 * NL, hipMemcpyHostToDevice, s));
    if (chi2_init) OV2_HIP_CHECK(hipMemcpyAsync(D.chi2, chi2_init, 8 * (size_t)dev->n_res, hipMemcpyHostToDevice, s));
    else OV2_HIP_CHECK(hipMemsetAsync(D.chi2, 0xFF, 8 * (size_t)std::max(1, dev->n_res), s));     // NaN pattern
    if (dpos_init) OV2_HIP_CHECK(hipMemcpyAsync(D.dpos, dpos_init, (size_t)dev->n_res, hipMemcpyHostToDevice, s));
    else OV2_HIP_CHECK(hipMemsetAsync(D.dpos, 0, (size_t)std::max(1, dev->n_res), s));
    }
    OV2_HIP_CHECK(hipEventRecord(e0, s));
    BACtl h_ctl;
    memset(&h_ctl, 0, sizeof(h_ctl));
    h_ctl.radius = o->initial_radius; h_ctl.decrease_factor = 2.0; h_ctl.x_norm = -1.0;
    h_ctl.need_lin = 1; h_ctl.step_successful = 1;
    h_ctl.termination = OV2_TERM_NO_CONVERGENCE;
    h_ctl.cur.gradient_norm = NAN;                          // (the device forms the max norm only)
    ctx->ba_trace_n = 0;
    if (ctx->ba_trace) {
        if (!ctx->ba_trace_d) OV2_HIP_CHECK(hipMalloc(&ctx->ba_trace_d, sizeof(BAIterRec) * BA_TRACE_CAP));
        if (!ctx->ba_trace_h) { ctx->ba_trace_h = malloc(sizeof(BAIterRec) * BA_TRACE_CAP); OV2_REQUIRE(ctx->ba_trace_h, OV2_ENOMEM, "trace buffer"); }
        h_ctl.trace = (BAIterRec *)ctx->ba_trace_d;
    }
    // one optimised pose, pose-only residual blocks, no landmarks (ceresPnP): the whole loop in one kernel (OV2_OPT_BA_POSE_ONLY_FUSED
    // = 0 keeps the multi-kernel path for A/B runs)
    const bool fused_po = fused_po_path;
    if (fused_po) {
        hipLaunchKernelGGL(k_ba_pose_only, dim3(1), dim3(256), 0, s, D, O, h_ctl);
        OV2_HIP_CHECK(hipGetLastError());
    } else {
    if (one_reset) {
        const int rb = (int)std::min<size_t>(256, ((size_t)std::max(std::max(D.n_res, D.nfp * D.nfp), D.n_lm) + 1023) / 1024);
        hipLaunchKernelGGL(k_ba_reset, dim3(std::max(1, rb)), dim3(256), 0, s, D, h_ctl, keep_state ? 1 : 0, (chi2_init || dpos_init) ? 1 : 0);
    } else {
    OV2_HIP_CHECK(hipMemcpyAsync(D.ctl, &h_ctl, sizeof(h_ctl), hipMemcpyHostToDevice, s));
    OV2_HIP_CHECK(hipMemsetAsync(D.H, 0, 8 * (size_t)D.nfp * D.nfp, s));
    OV2_HIP_CHECK(hipMemsetAsync(D.bf, 0, 8 * (size_t)D.nfp, s));
    OV2_HIP_CHECK(hipMemsetAsync(D.yf, 0, 8 * (size_t)D.nfp, s));
    }
    // poses -> R | t, scales = 1 (round 1 filled the scales through a host staging vector: three copies and a synchronisation)
    hipLaunchKernelGGL(k_ba_init, dim3((int)std::min<size_t>(1024, (std::max<size_t>(std::max<size_t>(D.n_kf, D.nfp), NL) + 255) / 256)), dim3(256), 0, s, D);

    const int lin_blocks = std::max(1, std::min(256, (D.n_lm + 15) / 16));   // (512: two workgroups per CU -- measured 15 % slower)
    const int ntiles = D.nfp / BA_TILE, n_upper = ntiles * (ntiles + 1) / 2;
    // rows of the W^T C W contraction: landmarks, or the 3 pseudo-rows per point of Wp (ldim 3)
    BADev DG = D;
    if (D.ldim == 3) { DG.W = D.Wp; DG.n_lm = 3 * D.n_lm; DG.cl = D.ones; DG.etb = D.ep; }
    int ksplit = std::max(1, std::min(64, (1024 + n_upper - 1) / n_upper));
    int lm_per_split = std::max(BA_TILE, ((DG.n_lm + ksplit - 1) / ksplit + BA_TILE - 1) / BA_TILE * BA_TILE);
    ksplit = std::max(1, (DG.n_lm + lm_per_split - 1) / lm_per_split);
    const int ws_blocks = std::max(1, std::min(512, std::max((D.n_lm + 3) / 4, (D.n_po + 255) / 256)));
    // inverse-depth form: 16 landmarks per work-group pass in the back-substitution, 8 in the cost kernel -- one pass each when the grid allows
    const int bs_blocks = std::max(1, std::min(2048, (D.n_lm + 15) / 16));
    const int cost_blocks = std::max(1, std::min(2048, std::max((D.n_lm + 7) / 8, (D.n_po + 255) / 256)));
    D.bs_blocks = bs_blocks; D.cost_blocks = cost_blocks; D.lin_blocks = lin_blocks;
    // OV2_OPT_BA_DETERMINISTIC (BADev::det): one-wavefront lineariser work-groups with their own copies of H / F^T b / cost, one copy
    // of W^T C W / v per landmark split; everything else of the solver is already a fixed-order computation
    int det_lin = 0, det_po = 0;
    if (ctx->ba_deterministic) {
        OV2_REQUIRE(D.ldim == 1 && !D.big, OV2_EUNSUPPORTED, "OV2_OPT_BA_DETERMINISTIC covers the inverse-depth form on the LDS-resident path only");
        det_lin = D.n_lm > 0 ? std::max(1, std::min(128, (D.n_lm + 15) / 16)) : 0;
        det_po = D.n_po > 0 ? std::max(1, std::min(32, (D.n_po + 63) / 64)) : 0;
        const size_t nn = (size_t)D.nfp * D.nfp, ncopy = (size_t)det_lin + det_po;
        const size_t b_H = al256(8 * ncopy * nn), b_bf = al256(8 * ncopy * D.nfp), b_c = al256(8 * std::max<size_t>(1, ncopy));
        const size_t b_G = al256(8 * (size_t)ksplit * nn), b_v = al256(8 * (size_t)ksplit * D.nfp);
        const size_t need = b_H + b_bf + b_c + b_G + b_v;
        // the copies live in the CONTEXT (grow-only, like d_scratch): ov2_local_ba / ov2_ba_solve create a transient problem per call
        if (need > ctx->ba_det_bytes) {
            if (ctx->ba_det_pool) { OV2_HIP_CHECK(hipStreamSynchronize(s)); (void)hipFree(ctx->ba_det_pool); ctx->ba_det_pool = nullptr; ctx->ba_det_bytes = 0; }
            hipError_t e = hipMalloc(&ctx->ba_det_pool, need);
            if (e != hipSuccess) { ov2_set_error("hipMalloc(%zu) for the deterministic mode: %s", need, hipGetErrorString(e)); return OV2_ENOMEM; }
            ctx->ba_det_bytes = need;
        }
        uint8_t *q = (uint8_t *)ctx->ba_det_pool;
        D.det = 1; D.det_lin = det_lin; D.det_po = det_po; D.det_ksplit = ksplit;
        D.Hpart = (double *)q; D.bfpart = (double *)(q + b_H); D.costpart = (double *)(q + b_H + b_bf);
        D.Gpart = (double *)(q + b_H + b_bf + b_c); D.vpart = (double *)(q + b_H + b_bf + b_c + b_G);
        OV2_HIP_CHECK(hipMemsetAsync(ctx->ba_det_pool, 0, b_H + b_bf + b_c, s));      // (the copies are clean between linearisations: k_ba_det_reduce clears as it reads)
        D.lin_blocks = det_lin;
        DG.det = 1; DG.det_ksplit = ksplit; DG.Gpart = D.Gpart; DG.vpart = D.vpart;
    }
    const int po_blocks = std::max(1, std::min(256, (D.n_po + 255) / 256));
    // k_ba_schur_sparse: ~512 work-groups; row block + per-wavefront staging (64 slot blocks + columns)
    const int ss_split = std::max(1, (512 + std::max(1, n_opt) - 1) / std::max(1, n_opt));
    // column chunk of the row block kept in LDS: all of it up to 2040 columns (340 pose blocks), else that many per chunk
    int ss_ncol = D.nfp <= 2048 ? D.nfp : 2040;
    if (ctx->ba_schur_chunk >= 6) ss_ncol = std::min(ss_ncol, ctx->ba_schur_chunk / 6 * 6);                                     // OV2_OPT_BA_SCHUR_CHUNK (tests)
    const int ss_chunks = (D.nfp + ss_ncol - 1) / ss_ncol;
    const size_t ss_lds = 8 * (6 * (size_t)ss_ncol + (size_t)SS_WAVES * 64 * 6) + 4 * (size_t)SS_WAVES * 64 + 64;

    auto linearize = [&]() {
        if (D.n_lm > 0 && D.ldim == 3) hipLaunchKernelGGL(k_ba_linearize_xyz, dim3(lin_blocks * (4 / D.lin_waves)), dim3(64 * D.lin_waves), lin_lds, s, D);
        else if (D.big) {
            // (k_ba_decide leaves H, F^T b and the W slots to this kernel on the large path: also for pose-only problems)
            if (D.n_lm > 0 || D.n_po > 0) hipLaunchKernelGGL(k_ba_zero_lin, dim3(1024), dim3(256), 0, s, D);
            if (D.n_lm > 0) hipLaunchKernelGGL(k_ba_linearize<true>, dim3(lin_blocks), dim3(256), lin_lds, s, D, dev->lm_order);
        }
        else if (D.det) {
            // one wavefront per work-group, each with its own copy of H / F^T b; then the copies in order
            if (D.n_lm > 0) hipLaunchKernelGGL(k_ba_linearize<false>, dim3(det_lin), dim3(64), lin_lds, s, D, dev->lm_order);
            if (D.n_po > 0) hipLaunchKernelGGL(k_ba_linearize_po, dim3(det_po), dim3(64), (size_t)n_opt * 27 * 8 + 16, s, D);
            hipLaunchKernelGGL(k_ba_det_reduce, dim3(256), dim3(256), 0, s, D);
            return;
        }
        else if (D.n_lm > 0) hipLaunchKernelGGL(k_ba_linearize<false>, dim3(lin_blocks), dim3(256), lin_lds, s, D, dev->lm_order);
        if (D.n_po > 0) hipLaunchKernelGGL(k_ba_linearize_po, dim3(po_blocks), dim3(256), (D.big && D.lin_direct ? 0 : (size_t)n_opt * 27 * 8) + 16, s, D);
    };
    linearize();
    if (!one_reset) OV2_HIP_CHECK(hipMemsetAsync(D.G, 0, 8 * (size_t)D.nfp * D.nfp, s));    // (every later iteration: cleared by the back-substitution kernel)
    // The LM loop is enqueued half an iteration ahead.  The first half of iteration `it` (bookkeeping, Schur complement, factorisation:
    // ~265 us of config 4's ~385) goes into the stream BEFORE the outcome of iteration it - 1 is known; k_ba_decide stores that outcome
    // into pinned host memory, and the second half (back-substitution .. decision, re-linearisation) follows when the host has seen
    // it -- while the GPU is still busy with the first half, so the stream never drains.  A solve that converges pays four empty
    // launches (every kernel starts with `if (ctl->done) return`): the two-iteration chunks of rounds 2-3 paid 18 plus a 4-byte
    // device-to-host copy + event per chunk, a whole iteration of look-ahead 9.
    int rc_h = ctx->reserve_host(64);
    if (rc_h != OV2_OK) return rc_h;
    volatile int *flag_h = (volatile int *)ctx->h_scratch;
    flag_h[0] = -1;
    D.flag_h = (int *)ctx->h_scratch;
    DG.flag_h = D.flag_h;
    auto first_half = [&](int it) {
        hipLaunchKernelGGL(k_ba_iter_begin, dim3(1), dim3(1024), 0, s, D, O, it);
        if (D.ldim == 3 && D.n_lm > 0) hipLaunchKernelGGL(k_ba_xyz_prep, dim3(ws_blocks), dim3(256), 0, s, D);
        if (D.n_lm > 0 && D.big) hipLaunchKernelGGL(k_ba_schur_sparse, dim3(n_opt * ss_split, ss_chunks), dim3(64 * SS_WAVES), ss_lds, s, D, ss_split, ss_ncol);
        else if (D.n_lm > 0) hipLaunchKernelGGL(k_ba_schur_gemm, dim3(n_upper, ksplit), dim3(256), 0, s, DG, ntiles, lm_per_split);
        if (D.nf > 0) hipLaunchKernelGGL(k_ba_assemble, dim3((D.nf + 255) / 256, D.nf), dim3(256), 0, s, D);   // (structure-only problems: no reduced system)
        if (D.chol_hbm) {
            for (int k0 = 0; k0 < D.nf; k0 += CH_NB) {
                const int m = D.nf - k0 - std::min(CH_NB, D.nf - k0);
                hipLaunchKernelGGL(k_chol_diag, dim3(1), dim3(64), 0, s, D, k0);
                if (m > 0) {
                    const int mb = (m + 31) / 32;
                    hipLaunchKernelGGL(k_chol_panel, dim3((m + 63) / 64), dim3(64), 0, s, D, k0);
                    hipLaunchKernelGGL(k_chol_trail, dim3(mb * (mb + 1) / 2), dim3(256), 0, s, D, k0);
                }
            }
            hipLaunchKernelGGL(k_chol_solve, dim3(1), dim3(512), chol_lds, s, D);
        } else
        hipLaunchKernelGGL(k_ba_cholesky, dim3(1), dim3(512), chol_lds, s, D);
    };
    auto second_half = [&](int it) {
        if (D.ldim == 3) hipLaunchKernelGGL(k_ba_backsub_xyz, dim3(ws_blocks), dim3(256), (size_t)D.nfp * 8, s, D);
        else hipLaunchKernelGGL(k_ba_backsub, dim3(bs_blocks), dim3(256), (size_t)D.nfp * 8, s, D);
        hipLaunchKernelGGL(k_ba_candidate, dim3(1), dim3(1024), 0, s, D, O);
        if (D.ldim == 3) hipLaunchKernelGGL(k_ba_cost_xyz, dim3(ws_blocks), dim3(256), 0, s, D);
        else hipLaunchKernelGGL(k_ba_cost, dim3(cost_blocks), dim3(256), 0, s, D);
        hipLaunchKernelGGL(k_ba_decide, dim3(1), dim3(1024), 0, s, D, O, it);
        linearize();
    };
    const auto t_start = std::chrono::steady_clock::now();
    for (int it = 0; it < o->max_iter; it++) {
        if (it > 0 && o->max_solver_time_s > 0.0) {
            // Ceres tests total_time >= max_solver_time_in_seconds at the top of every iteration; here against the time the DEVICE
            // has actually spent (wait for the previous iteration first, otherwise only the enqueue is timed)
            OV2_HIP_CHECK(hipStreamSynchronize(s));
            const double el = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count();
            if (el >= o->max_solver_time_s) {
                // the regular per-iteration bookkeeping with an iteration budget of zero: it finalises the last step (successful
                // step count, minimum cost, cost of a fresh linearisation) and terminates with NO_CONVERGENCE
                BAOpt Ostop = O;
                Ostop.max_iter = 0;
                hipLaunchKernelGGL(k_ba_iter_begin, dim3(1), dim3(1024), 0, s, D, Ostop, -1);
                break;
            }
        }
        first_half(it);
        if (it >= 1) {
            // outcome of iteration it - 1 (k_ba_decide of that iteration)
            unsigned spins = 0;
            while (flag_h[0] < 2 * (it - 1)) {
#if !defined(__HIP_DEVICE_COMPILE__) && defined(__x86_64__)
                __builtin_ia32_pause();                                               // the estimator thread shares its core's siblings with the SLAM / mapper threads
#endif
                if ((++spins & 0x3FFFFFu) == 0) {                                 // (a watchdog, ~every 0.3 s: a query per wait put a 6 us bubble in front of the next launch)
                    const hipError_t q = hipStreamQuery(s);
                    if (q == hipSuccess) break;                               // everything enqueued has run: the word is final
                    if (q != hipErrorNotReady) OV2_HIP_CHECK(q);
                }
            }
            if (flag_h[0] >= 0 && (flag_h[0] & 1)) break;
        }
        second_half(it);
    }
    hipLaunchKernelGGL(k_ba_iter_begin, dim3(1), dim3(1024), 0, s, D, O, -1);    // final bookkeeping
    OV2_HIP_CHECK(hipGetLastError());
    }
    OV2_HIP_CHECK(hipEventRecord(e1, s));
    // results
    OV2_HIP_CHECK(hipMemcpyAsync(&h_ctl, D.ctl, sizeof(h_ctl), hipMemcpyDeviceToHost, s));
    if (r->poses_out) OV2_HIP_CHECK(hipMemcpyAsync(r->poses_out, D.x_pose, 56 * (size_t)D.n_kf, hipMemcpyDeviceToHost, s));
    if (r->invdepth_out && D.n_lm > 0) OV2_HIP_CHECK(hipMemcpyAsync(r->invdepth_out, D.x_lam, 8 * NL, hipMemcpyDeviceToHost, s));
    if (r->chi2_last_eval && dev->n_res > 0) OV2_HIP_CHECK(hipMemcpyAsync(r->chi2_last_eval, D.chi2, 8 * (size_t)dev->n_res, hipMemcpyDeviceToHost, s));
    if (r->depthpos_last_eval && dev->n_res > 0) OV2_HIP_CHECK(hipMemcpyAsync(r->depthpos_last_eval, D.dpos, (size_t)dev->n_res, hipMemcpyDeviceToHost, s));
    OV2_HIP_CHECK(hipStreamSynchronize(s));
    if (h_ctl.trace) {
        ctx->ba_trace_n = h_ctl.n_trace;
        const int nrec = std::min(h_ctl.n_trace, BA_TRACE_CAP);
        if (nrec > 0) OV2_HIP_CHECK(hipMemcpy(ctx->ba_trace_h, ctx->ba_trace_d, sizeof(BAIterRec) * (size_t)nrec, hipMemcpyDeviceToHost));
    }
    float ms = 0;
    OV2_HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
    r->iterations = h_ctl.n_steps; r->num_successful_steps = h_ctl.n_success;
    r->initial_cost = h_ctl.initial_cost; r->final_cost = h_ctl.minimum_cost; r->termination = h_ctl.termination;
    r->solve_ms = ms;
    if (ctx->debug)
        fprintf(stderr, "[ov2 ba] cholesky ticks (100MHz): copy-in %llu pivot+panel %llu write-back %llu trailing %llu block inverses %llu solves %llu\n",
                h_ctl.dbg[0], h_ctl.dbg[1], h_ctl.dbg[2], h_ctl.dbg[3], h_ctl.dbg[4], h_ctl.dbg[5]);
    return OV2_OK;
}


// ================================================================================== lock-step batch of local-BA problems
// BASELINE configs[4]: eleven sequences advance in lock step on one GPU (ov2_btracker_*), their keyframes arrive together -- and
// eleven estimator threads with a stream each then push ~100 launches per solve through the command processor, where they queue
// behind each other and behind the front end's (round 5: 5.8 ms of wall clock per 0.9 ms solve, the SLAM thread 1.8x slower).
// Here the problems of one step share every launch: blockIdx.z = problem, the kernels read their BADev from an array in device
// memory instead of the kernel arguments, a problem that has converged (or takes no second pass) leaves through the kernels'
// `if (ctl->done) return`.  The one-work-group kernels (factorisation, bookkeeping) so run on as many CUs as there are problems.
// The arithmetic of a problem is that of ov2_local_ba (same device functions); grids are the largest any problem of the batch
// needs, the per-work-group partial sums are added in a different grouping when a problem runs on a larger grid than alone.

// results of the batch into ONE block (poses | inverse depths | outlier verdicts [| chi2] [| depth flags] per problem, 256-byte
// aligned parts): one download instead of three to five small ones per problem
__global__ __launch_bounds__(256) void k_ba_gather_B(const BADev *__restrict__ arr)
{
    const BADev &D = arr[blockIdx.z];
    const long long i0 = (long long)blockIdx.x * blockDim.x + threadIdx.x, stride = (long long)gridDim.x * blockDim.x;
    uint8_t *o = D.out_b;
    for (long long e = i0; e < 7LL * D.n_kf; e += stride) ((double *)o)[e] = D.x_pose[e];
    o += (56 * (size_t)D.n_kf + 255) & ~(size_t)255;
    for (long long e = i0; e < D.n_lm; e += stride) ((double *)o)[e] = D.x_lam[e];
    o += (8 * (size_t)max(1, D.n_lm) + 255) & ~(size_t)255;
    for (long long e = i0; e < D.n_res; e += stride) o[e] = D.bad_obs[e];
    o += ((size_t)D.n_res + 255) & ~(size_t)255;
    if (D.out_flags & 1) { for (long long e = i0; e < D.n_res; e += stride) ((double *)o)[e] = D.chi2[e]; o += (8 * (size_t)D.n_res + 255) & ~(size_t)255; }
    if (D.out_flags & 2) for (long long e = i0; e < D.n_res; e += stride) o[e] = D.dpos[e];
}

static bool ba_small_path(int n_opt)
{
    const int nf = 6 * n_opt, nfp = std::max(BA_TILE, (nf + BA_TILE - 1) / BA_TILE * BA_TILE);
    const size_t lin_lds = 8 * (8 * (size_t)nfp + (size_t)n_opt * 27 + 4 * (size_t)n_opt * 21 + 4 * (size_t)LIN_RED) + 64;
    return !(lin_lds > 159 * 1024 || chol_lds_bytes(nf, nfp) > 150 * 1024 || nf > CH_MAX_LDS_N);
}

struct BABatch {
    std::vector<ov2_ba_dev *> devs;
    BADev *h_arr = nullptr, *d_arr = nullptr;           // the problems' device views: pinned staging / device copy
    BACtl *h_ctl = nullptr, *d_ctl = nullptr;           // control blocks, consecutive (one download per pass)
    int *h_cnt = nullptr, *d_cnt = nullptr;             // 16 counters per problem (k_ba_mark_outliers)
    volatile int *h_flag = nullptr;                     // the look-ahead words of k_ba_decide
    bool lm_live_first = false;                         // second pass: landmarks that lost all their blocks leave the program first
    ~BABatch() { for (ov2_ba_dev *d : devs) ba_destroy(d); }
};

// one LM solve of every problem of the batch (ba_run's loop on batched launches); skip[i]: the problem sits this pass out
static int ba_run_batch(ov2_ctx *ctx, BABatch &B, const ov2_ba_options *o, const double *huber, const uint8_t *skip, bool keep_state, float *ms_out)
{
    OV2_REQUIRE(o->max_iter >= 0 && o->initial_radius > 0 && o->min_lm_diagonal > 0 && o->min_lm_diagonal <= o->max_lm_diagonal,
                OV2_EINVAL, "bad solver options");
    const int N = (int)B.devs.size();
    hipStream_t s = ctx->stream;
    BAOpt O;
    O.max_iter = o->max_iter; O.ftol = o->function_tolerance; O.gtol = o->gradient_tolerance; O.ptol = o->parameter_tolerance;
    O.max_radius = o->max_radius; O.min_radius = o->min_radius; O.min_diag = o->min_lm_diagonal; O.max_diag = o->max_lm_diagonal;
    O.min_rel_decrease = o->min_relative_decrease; O.jacobi = o->jacobi_scaling; O.max_invalid = o->max_consecutive_invalid_steps;
    int lin_blocks = 1, bs_blocks = 1, cost_blocks = 1, nupper = 1, ksplit_max = 1, nf_max = 0, nfp_max = 0, reset_blocks = 1, init_blocks = 1;
    size_t lin_lds = 0, chol_lds = 0;
    // a single problem spreads over the whole chip for latency (16 landmarks per lineariser work-group, 1024 Schur work-groups); a batch
    // fills it anyway: ~768 lineariser and ~2048 Schur work-groups over ALL problems -- fewer flushes of the LDS aggregates and fewer
    // atomic adds into G per problem (eleven windows: 2.31 -> 2.07 ms of device time; tools/r5_ba_batch_grid.sh swept 512 .. 4096 / 1024 .. 16384)
    const int lin_total = 768, schur_total = 2048;
    const int lin_cap = std::max(16, std::min(256, (lin_total + N - 1) / N));
    const int schur_wgs = std::max(64, std::min(1024, (schur_total + N - 1) / N));
    for (int i = 0; i < N; i++) {
        const BADev &D = B.devs[(size_t)i]->D;
        const int n_opt = D.nf / 6;
        lin_lds = std::max(lin_lds, 8 * (8 * (size_t)D.nfp + (size_t)n_opt * 27 + 4 * (size_t)n_opt * 21 + 4 * (size_t)LIN_RED) + 64);
        chol_lds = std::max(chol_lds, chol_lds_bytes(D.nf, D.nfp));
        lin_blocks = std::max(lin_blocks, std::min(lin_cap, (D.n_lm + 15) / 16));
        bs_blocks = std::max(bs_blocks, std::min(2048, (D.n_lm + 15) / 16));
        cost_blocks = std::max(cost_blocks, std::min(2048, (D.n_lm + 7) / 8));
        nf_max = std::max(nf_max, D.nf); nfp_max = std::max(nfp_max, D.nfp);
        reset_blocks = std::max(reset_blocks, (int)std::min<size_t>(256, ((size_t)std::max(D.n_res, D.nfp * D.nfp) + 1023) / 1024));
        init_blocks = std::max(init_blocks, (int)std::min<size_t>(1024, ((size_t)std::max(std::max(D.n_kf, D.nfp), D.n_lm) + 255) / 256));
    }
    OV2_REQUIRE(lin_lds <= 159 * 1024 && chol_lds <= 150 * 1024, OV2_EUNSUPPORTED, "a problem of the batch is too large for the LDS-resident path");
    for (int i = 0; i < N; i++) {
        BADev D = B.devs[(size_t)i]->D;
        D.huber = huber[i]; D.min_diag = o->min_lm_diagonal; D.max_diag = o->max_lm_diagonal;
        D.bs_blocks = bs_blocks; D.cost_blocks = cost_blocks; D.lin_blocks = lin_blocks;
        const int ntiles = D.nfp / BA_TILE, n_upper = ntiles * (ntiles + 1) / 2;
        int ksplit = std::max(1, std::min(64, (schur_wgs + n_upper - 1) / n_upper));
        const int lmps = std::max(BA_TILE, ((D.n_lm + ksplit - 1) / ksplit + BA_TILE - 1) / BA_TILE * BA_TILE);
        ksplit = std::max(1, (D.n_lm + lmps - 1) / lmps);
        D.g_ntiles = ntiles; D.g_nupper = n_upper; D.g_lmps = lmps; D.g_ksplit = ksplit;
        nupper = std::max(nupper, n_upper); ksplit_max = std::max(ksplit_max, ksplit);
        D.skip2 = skip && skip[i] ? 1 : 0;
        D.flag_h = (int *)(B.h_flag + i);
        D.ctl = B.d_ctl + i; D.lba_cnt = B.d_cnt + 16 * i;
        B.h_arr[i] = D;
        B.h_flag[i] = -1;
    }
    OV2_HIP_CHECK(hipMemcpyAsync(B.d_arr, B.h_arr, sizeof(BADev) * (size_t)N, hipMemcpyHostToDevice, s));
    for (int i = 0; i < 2; i++) if (!ctx->ba_ev[i]) OV2_HIP_CHECK(hipEventCreate(&ctx->ba_ev[i]));
    struct { hipEvent_t e0, e1; } ev{ctx->ba_ev[0], ctx->ba_ev[1]};
    OV2_HIP_CHECK(hipEventRecord(ev.e0, s));
    BACtl c0;
    memset(&c0, 0, sizeof(c0));
    c0.radius = o->initial_radius; c0.decrease_factor = 2.0; c0.x_norm = -1.0;
    c0.need_lin = 1; c0.step_successful = 1; c0.termination = OV2_TERM_NO_CONVERGENCE;
    const BADev *A = B.d_arr;
    const unsigned Z = (unsigned)N;
    if (B.lm_live_first) {
        int ll = 1;
        for (int i = 0; i < N; i++) ll = std::max(ll, std::min(512, (B.devs[(size_t)i]->D.n_lm + 3) / 4));
        hipLaunchKernelGGL(k_ba_lm_live_B, dim3(ll, 1, Z), dim3(256), 0, s, A);
    }
    hipLaunchKernelGGL(k_ba_reset_B, dim3(reset_blocks, 1, Z), dim3(256), 0, s, A, c0, keep_state ? 1 : 0);
    hipLaunchKernelGGL(k_ba_init_B, dim3(init_blocks, 1, Z), dim3(256), 0, s, A);
    auto linearize = [&]() { hipLaunchKernelGGL(k_ba_linearize_B, dim3(lin_blocks, 1, Z), dim3(256), lin_lds, s, A); };
    auto first_half = [&](int it) {
        hipLaunchKernelGGL(k_ba_iter_begin_B, dim3(1, 1, Z), dim3(1024), 0, s, A, O, it);
        hipLaunchKernelGGL(k_ba_schur_gemm_B, dim3(nupper, ksplit_max, Z), dim3(256), 0, s, A);
        hipLaunchKernelGGL(k_ba_assemble_B, dim3((nf_max + 255) / 256, nf_max, Z), dim3(256), 0, s, A);
        hipLaunchKernelGGL(k_ba_cholesky_B, dim3(1, 1, Z), dim3(512), chol_lds, s, A);
    };
    auto second_half = [&](int it) {
        hipLaunchKernelGGL(k_ba_backsub_B, dim3(bs_blocks, 1, Z), dim3(256), (size_t)nfp_max * 8, s, A);
        hipLaunchKernelGGL(k_ba_candidate_B, dim3(1, 1, Z), dim3(1024), 0, s, A, O);
        hipLaunchKernelGGL(k_ba_cost_B, dim3(cost_blocks, 1, Z), dim3(256), 0, s, A);
        hipLaunchKernelGGL(k_ba_decide_B, dim3(1, 1, Z), dim3(1024), 0, s, A, O, it);
        linearize();
    };
    linearize();
    const auto t_start = std::chrono::steady_clock::now();
    for (int it = 0; it < o->max_iter; it++) {
        if (it > 0 && o->max_solver_time_s > 0.0) {
            // (the budget of ba_run, against the time the device has spent on the batch)
            OV2_HIP_CHECK(hipStreamSynchronize(s));
            if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count() >= o->max_solver_time_s) {
                BAOpt Ostop = O;
                Ostop.max_iter = 0;
                hipLaunchKernelGGL(k_ba_iter_begin_B, dim3(1, 1, Z), dim3(1024), 0, s, A, Ostop, -1);
                break;
            }
        }
        first_half(it);
        if (it >= 1) {
            // the outcome of iteration it - 1 of EVERY problem (a finished problem's k_ba_decide reports `done` on its way out)
            unsigned spins = 0;
            bool all_done = false;
            for (;;) {
                int known = 0, done = 0;
                for (int i = 0; i < N; i++) { const int f = B.h_flag[i]; known += f >= 2 * (it - 1); done += f >= 0 && (f & 1); }
                if (known == N) { all_done = done == N; break; }
#if !defined(__HIP_DEVICE_COMPILE__) && defined(__x86_64__)
                __builtin_ia32_pause();
#endif
                if ((++spins & 0xFFFFFu) == 0) {
                    const hipError_t q = hipStreamQuery(s);
                    if (q == hipSuccess) {
                        all_done = true;
                        for (int i = 0; i < N; i++) all_done = all_done && B.h_flag[i] >= 0 && (B.h_flag[i] & 1);
                        break;
                    }
                    if (q != hipErrorNotReady) OV2_HIP_CHECK(q);
                }
            }
            if (all_done) break;
        }
        second_half(it);
    }
    hipLaunchKernelGGL(k_ba_iter_begin_B, dim3(1, 1, Z), dim3(1024), 0, s, A, O, -1);    // final bookkeeping
    OV2_HIP_CHECK(hipGetLastError());
    OV2_HIP_CHECK(hipEventRecord(ev.e1, s));
    OV2_HIP_CHECK(hipMemcpyAsync(B.h_ctl, B.d_ctl, sizeof(BACtl) * (size_t)N, hipMemcpyDeviceToHost, s));
    OV2_HIP_CHECK(hipStreamSynchronize(s));
    OV2_HIP_CHECK(hipEventElapsedTime(ms_out, ev.e0, ev.e1));
    return OV2_OK;
}

static bool same_solver_options(const ov2_ba_options &a, const ov2_ba_options &b)
{
    return a.max_iter == b.max_iter && a.function_tolerance == b.function_tolerance && a.gradient_tolerance == b.gradient_tolerance &&
           a.parameter_tolerance == b.parameter_tolerance && a.initial_radius == b.initial_radius && a.max_radius == b.max_radius &&
           a.min_radius == b.min_radius && a.min_lm_diagonal == b.min_lm_diagonal && a.max_lm_diagonal == b.max_lm_diagonal &&
           a.min_relative_decrease == b.min_relative_decrease && a.jacobi_scaling == b.jacobi_scaling &&
           a.max_consecutive_invalid_steps == b.max_consecutive_invalid_steps && a.max_solver_time_s == b.max_solver_time_s;
}

static int local_ba_batch(ov2_ctx *ctx, int n, const ov2_ba_problem *p, const ov2_local_ba_options *o, ov2_local_ba_result *r, int *n_batched)
{
    OV2_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    for (int i = 0; i < n; i++) {
        OV2_REQUIRE(o[i].robust_mono_th > 0, OV2_EINVAL, "robust_mono_th must be positive");
        OV2_REQUIRE(o[i].robust_mono_th == o[0].robust_mono_th && o[i].use_robust_cost == o[0].use_robust_cost && o[i].apply_l2_after_robust == o[0].apply_l2_after_robust &&
                    same_solver_options(o[i].pass1, o[0].pass1) && same_solver_options(o[i].pass2, o[0].pass2), OV2_EINVAL,
                    "ov2_local_ba_batch: the problems of a batch share the protocol and solver options (only the stop request is per problem)");
        ov2_local_ba_result &ri = r[i];
        ri.l2_done = 0; ri.pass2_error = OV2_OK; ri.n_bad_pass1 = 0; ri.n_bad_total = 0; ri.status = OV2_OK;
        for (int q = 0; q < 2; q++) { ri.iterations[q] = 0; ri.num_successful_steps[q] = 0; ri.termination[q] = OV2_TERM_NO_CONVERGENCE; ri.initial_cost[q] = ri.final_cost[q] = 0; ri.solve_ms[q] = 0; }
    }
    // which problems can share launches: inverse-depth problems of the LDS-resident path with landmarks and optimised keyframes
    std::vector<int> idx;                                   // batch slot -> problem
    std::vector<uint8_t> alone((size_t)n, 0);
    for (int i = 0; i < n; i++) {
        int n_opt = 0;
        if (p[i].n_kf > 0 && p[i].kf_const) for (int k = 0; k < p[i].n_kf; k++) n_opt += !p[i].kf_const[k];
        const bool ok = !ctx->ba_deterministic && !ctx->ba_force_large && p[i].n_lm > 0 && p[i].n_res > 0 && n_opt > 0 && ba_small_path(n_opt);
        if (ok) idx.push_back(i); else alone[(size_t)i] = 1;
    }
    BABatch B;
    int N = (int)idx.size();
    const bool dbg = ctx->debug != 0;
    const auto tw0 = std::chrono::steady_clock::now();
    auto lap = [&](const char *what) {
        if (dbg) fprintf(stderr, "[ov2 local_ba_batch] %-28s %8.3f ms since entry (%d problems)\n", what, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tw0).count(), N);
    };
    size_t out_base = 0, out_total = 0;                     // the batch's result block (k_ba_gather_B) inside the header
    std::vector<size_t> out_off;
    if (N > 0) {
        // header of the pinned block: look-ahead words, counters, control blocks, device views; then the staging mirrors
        const size_t hb_flag = 0, hb_cnt = al256(4 * (size_t)N), hb_ctl = hb_cnt + al256(64 * (size_t)N), hb_arr = hb_ctl + al256(sizeof(BACtl) * (size_t)N);
        out_base = hb_arr + al256(sizeof(BADev) * (size_t)N);
        out_off.assign(idx.size(), 0);
        for (size_t k = 0; k < idx.size(); k++) {
            const ov2_ba_problem &q = p[idx[k]];
            const size_t nk = (size_t)std::max(0, q.n_kf), nl = (size_t)std::max(1, q.n_lm), nr = (size_t)std::max(0, q.n_res);
            out_off[k] = out_total;
            out_total += al256(56 * nk) + al256(8 * nl) + al256(nr) + (r[idx[k]].chi2_last_eval ? al256(8 * nr) : 0) + (r[idx[k]].depthpos_last_eval ? al256(nr) : 0);
        }
        const size_t header = out_base + al256(out_total);          // (look-ahead words | counters | control blocks | views | results), then the problems' slices
        size_t host_need = header, dev_need = header;
        for (;;) {
            int rc = ctx->reserve_host(std::max(host_need, ctx->h_scratch_bytes));
            if (rc == OV2_OK) rc = ctx->reserve_device(std::max(dev_need, ctx->d_scratch_bytes));
            if (rc != OV2_OK) return rc;
            uint8_t *hb = (uint8_t *)ctx->h_scratch, *db = (uint8_t *)ctx->d_scratch;
            B.h_flag = (volatile int *)(hb + hb_flag); B.h_cnt = (int *)(hb + hb_cnt); B.h_ctl = (BACtl *)(hb + hb_ctl); B.h_arr = (BADev *)(hb + hb_arr);
            B.d_cnt = (int *)(db + hb_cnt); B.d_ctl = (BACtl *)(db + hb_ctl); B.d_arr = (BADev *)(db + hb_arr);
            BASlice sl;
            sl.dev_base = db; sl.dev_cap = ctx->d_scratch_bytes; sl.dev_used = header; sl.host_base = hb; sl.host_cap = ctx->h_scratch_bytes; sl.host_used = header;
            // the host side of a problem (validation, the landmark sort, the staging mirror; ~0.4 ms for a 69 k-block window) on a thread of
            // its own (sixteen persistent threads of the context) -- on one thread it was more than the batch's device time.  Each thread enqueues its
            // problem's upload on the context's stream itself (the order of the uploads does not matter).
            std::vector<ov2_ba_dev *> made(idx.size(), nullptr);
            std::vector<int> rcs(idx.size(), OV2_OK);
            std::vector<std::string> errs(idx.size());
            BAHostPool *hp = idx.size() > 1 ? ba_host_pool_of(ctx) : nullptr;
            const std::function<void(int)> work = [&](int k) {
                (void)hipSetDevice(ctx->device);
                rcs[(size_t)k] = ba_create(ctx, &p[idx[(size_t)k]], &made[(size_t)k], true, &sl);
                if (rcs[(size_t)k] != OV2_OK && rcs[(size_t)k] != BA_SLICE_FULL) errs[(size_t)k] = ov2_last_error();          // (the message is per thread)
            };
            if (hp) hp->run((int)idx.size(), work);
            else for (size_t k = 0; k < idx.size(); k++) work((int)k);
            bool full = false;
            int bad_rc = OV2_OK; size_t bad_k = 0;
            for (size_t k = 0; k < idx.size(); k++) {
                if (rcs[k] == BA_SLICE_FULL) full = true;
                else if (rcs[k] != OV2_OK && bad_rc == OV2_OK) { bad_rc = rcs[k]; bad_k = k; }
            }
            if (bad_rc == OV2_OK && !full) {
                for (size_t k = 0; k < idx.size(); k++) {
                    made[k]->D.out_b = db + out_base + out_off[k];
                    made[k]->D.out_flags = (r[idx[k]].chi2_last_eval ? 1 : 0) | (r[idx[k]].depthpos_last_eval ? 2 : 0);
                }
                B.devs = made;
                break;
            }
            OV2_HIP_CHECK(hipStreamSynchronize(s));
            for (ov2_ba_dev *d : made) ba_destroy(d);
            if (bad_rc != OV2_OK) { ov2_set_error("ov2_local_ba_batch: problem %d: %s", idx[bad_k], errs[bad_k].c_str()); return bad_rc; }
            // grow-only blocks: twice what this batch would have taken, and start over (the first batches of a run only)
            host_need = 2 * sl.host_used; dev_need = 2 * sl.dev_used;
        }
        // problems that turn out to carry pose-only blocks leave the batch
        for (size_t k = 0; k < B.devs.size();) {
            if (B.devs[k]->D.n_po > 0 || B.devs[k]->D.big) { alone[(size_t)idx[k]] = 1; OV2_HIP_CHECK(hipStreamSynchronize(s)); ba_destroy(B.devs[k]); B.devs.erase(B.devs.begin() + (long)k); idx.erase(idx.begin() + (long)k); out_off.erase(out_off.begin() + (long)k); }
            else k++;
        }
        N = (int)idx.size();
    }
    if (n_batched) *n_batched = N;
    lap("sort + upload (ba_create)");
    if (N > 0) {
        const ov2_local_ba_options &o0 = o[0];
        const double hub = o0.use_robust_cost ? sqrt(o0.robust_mono_th) : -1.0;
        std::vector<double> huber((size_t)N, hub);
        std::vector<uint8_t> skip((size_t)N, 0);
        OV2_HIP_CHECK(hipMemsetAsync(B.d_cnt, 0, 64 * (size_t)N, s));
        ov2_ba_options o1 = o0.pass1;
        float ms = 0;
        int rc = ba_run_batch(ctx, B, &o1, huber.data(), nullptr, false, &ms);
        if (rc != OV2_OK) return rc;
        lap("pass 1");
        for (int k = 0; k < N; k++) {
            ov2_local_ba_result &ri = r[idx[(size_t)k]];
            const BACtl &c = B.h_ctl[k];
            ri.iterations[0] = c.n_steps; ri.num_successful_steps[0] = c.n_success; ri.termination[0] = c.termination;
            ri.initial_cost[0] = c.initial_cost; ri.final_cost[0] = c.minimum_cost; ri.solve_ms[0] = ms;
        }
        int mk_blocks = 1;
        for (int k = 0; k < N; k++) mk_blocks = std::max(mk_blocks, std::min(1024, (B.devs[(size_t)k]->D.n_act + 255) / 256));
        hipLaunchKernelGGL(k_ba_mark_outliers_B, dim3(mk_blocks, 1, (unsigned)N), dim3(256), 0, s, (const BADev *)B.d_arr, o0.robust_mono_th, o0.apply_l2_after_robust ? 1 : 0, (uint8_t *)nullptr);
        OV2_HIP_CHECK(hipGetLastError());
        OV2_HIP_CHECK(hipMemcpyAsync(B.h_cnt, B.d_cnt, 64 * (size_t)N, hipMemcpyDeviceToHost, s));
        for (int k = 0; k < N; k++) {
            ov2_local_ba_result &ri = r[idx[(size_t)k]];
            const ov2_ba_dev *dev = B.devs[(size_t)k];
            if (ri.bad_after_pass1 && dev->n_res > 0) OV2_HIP_CHECK(hipMemcpyAsync(ri.bad_after_pass1, dev->D.bad_obs, (size_t)dev->n_res, hipMemcpyDeviceToHost, s));
        }
        OV2_HIP_CHECK(hipStreamSynchronize(s));
        lap("outlier test 1");
        // the stop request of each problem is read HERE, after its first solve (src/optimizer.cpp:603-604)
        int n_pass2 = 0;
        std::vector<int> bad1((size_t)N, 0);
        for (int k = 0; k < N; k++) {
            const ov2_local_ba_options &ok = o[idx[(size_t)k]];
            ov2_local_ba_result &ri = r[idx[(size_t)k]];
            const int nbbad = B.h_cnt[16 * k], left = B.h_cnt[16 * k + 1], right = B.h_cnt[16 * k + 2];
            bad1[(size_t)k] = nbbad; ri.n_bad_pass1 = nbbad; ri.n_bad_total = nbbad;
            const bool stop = ok.stop_requested || (ok.stop_flag && *ok.stop_flag);
            const bool go = o0.apply_l2_after_robust && o0.use_robust_cost && !stop && nbbad > 0;
            skip[(size_t)k] = go ? 0 : 1;
            huber[(size_t)k] = (left && right) ? -1.0 : hub;                   // (:606-608: mono runs keep Huber)
            n_pass2 += go;
        }
        if (n_pass2 > 0) {
            // (skip2 reaches the device with ba_run_batch's upload of the views: k_ba_lm_live_B runs after it, as part of the reset)
            OV2_HIP_CHECK(hipMemsetAsync(B.d_cnt, 0, 64 * (size_t)N, s));
            ov2_ba_options o2 = o0.pass2;
            B.lm_live_first = true;
            rc = ba_run_batch(ctx, B, &o2, huber.data(), skip.data(), true, &ms);
            B.lm_live_first = false;
            lap("pass 2");
            if (rc != OV2_OK) {
                for (int k = 0; k < N; k++) if (!skip[(size_t)k]) r[idx[(size_t)k]].pass2_error = rc;
            } else {
                for (int k = 0; k < N; k++) {
                    if (skip[(size_t)k]) continue;
                    ov2_local_ba_result &ri = r[idx[(size_t)k]];
                    const BACtl &c = B.h_ctl[k];
                    ri.l2_done = 1;
                    ri.iterations[1] = c.n_steps; ri.num_successful_steps[1] = c.n_success; ri.termination[1] = c.termination;
                    ri.initial_cost[1] = c.initial_cost; ri.final_cost[1] = c.minimum_cost; ri.solve_ms[1] = ms;
                }
                hipLaunchKernelGGL(k_ba_mark_outliers_B, dim3(mk_blocks, 1, (unsigned)N), dim3(256), 0, s, (const BADev *)B.d_arr, o0.robust_mono_th, 0, (uint8_t *)nullptr);
                OV2_HIP_CHECK(hipGetLastError());
                OV2_HIP_CHECK(hipMemcpyAsync(B.h_cnt, B.d_cnt, 64 * (size_t)N, hipMemcpyDeviceToHost, s));
            }
        }
        {
            int gb = 1;
            for (int k = 0; k < N; k++) gb = std::max(gb, std::min(64, (std::max(B.devs[(size_t)k]->D.n_res, B.devs[(size_t)k]->D.n_lm) + 1023) / 1024));
            hipLaunchKernelGGL(k_ba_gather_B, dim3(gb, 1, (unsigned)N), dim3(256), 0, s, (const BADev *)B.d_arr);
            OV2_HIP_CHECK(hipGetLastError());
            uint8_t *hb = (uint8_t *)ctx->h_scratch, *db = (uint8_t *)ctx->d_scratch;
            OV2_HIP_CHECK(hipMemcpyAsync(hb + out_base, db + out_base, out_total, hipMemcpyDeviceToHost, s));
            OV2_HIP_CHECK(hipStreamSynchronize(s));
            for (int k = 0; k < N; k++) {
                ov2_local_ba_result &ri = r[idx[(size_t)k]];
                const BADev &D = B.devs[(size_t)k]->D;
                const uint8_t *o = hb + out_base + out_off[(size_t)k];
                const size_t nr = (size_t)D.n_res;
                if (ri.poses_out) memcpy(ri.poses_out, o, 56 * (size_t)D.n_kf);
                o += al256(56 * (size_t)D.n_kf);
                if (ri.invdepth_out) memcpy(ri.invdepth_out, o, 8 * (size_t)D.n_lm);
                o += al256(8 * (size_t)std::max(1, D.n_lm));
                if (ri.bad_obs && nr > 0) memcpy(ri.bad_obs, o, nr);
                o += al256(nr);
                if (ri.chi2_last_eval) { if (nr > 0) memcpy(ri.chi2_last_eval, o, 8 * nr); o += al256(8 * nr); }
                if (ri.depthpos_last_eval && nr > 0) memcpy(ri.depthpos_last_eval, o, nr);
            }
        }
        lap("outlier test 2 + download");
        for (int k = 0; k < N; k++) if (r[idx[(size_t)k]].l2_done) r[idx[(size_t)k]].n_bad_total = bad1[(size_t)k] + B.h_cnt[16 * k];
        for (ov2_ba_dev *d : B.devs) ba_destroy(d);
        B.devs.clear();
    }
    // what cannot share launches (large windows, pose-only blocks, the deterministic mode): one problem at a time
    // every one of them is attempted: r[i].status says which results are valid, the call returns the first failure
    int first_err = OV2_OK;
    for (int i = 0; i < n; i++) {
        if (!alone[(size_t)i]) continue;
        const int rc = ov2_local_ba(ctx, &p[i], &o[i], &r[i]);
        r[i].status = rc;
        if (rc != OV2_OK && first_err == OV2_OK) first_err = rc;
    }
    return first_err;
}

extern "C" {

void ov2_ba_default_options(ov2_ba_options *o)
{
    if (!o) return;
    o->max_iter = 5; o->function_tolerance = 1e-3; o->gradient_tolerance = 1e-10; o->parameter_tolerance = 1e-8;
    o->huber_delta = sqrt(5.9915); o->initial_radius = 1e4; o->max_radius = 1e16; o->min_radius = 1e-32;
    o->min_lm_diagonal = 1e-6; o->max_lm_diagonal = 1e32; o->min_relative_decrease = 1e-3; o->jacobi_scaling = 1;
    o->max_consecutive_invalid_steps = 5;
    o->max_solver_time_s = 0.0;
}

int ov2_ba_get_trace(ov2_ctx *ctx, ov2_ba_iter *buf, int cap, int *n)
{
    OV2_REQUIRE(ctx && n && cap >= 0 && (cap == 0 || buf), OV2_EINVAL, "NULL argument");
    *n = ctx->ba_trace_n;
    const int k = std::min(std::min(ctx->ba_trace_n, BA_TRACE_CAP), cap);
    if (k > 0) memcpy(buf, ctx->ba_trace_h, sizeof(ov2_ba_iter) * (size_t)k);
    return OV2_OK;
}

int ov2_ba_solve(ov2_ctx *ctx, const ov2_ba_problem *p, const ov2_ba_options *o, ov2_ba_result *r)
{
    OV2_REQUIRE(ctx && p && o && r, OV2_EINVAL, "NULL argument");
    ov2_ba_dev *dev = nullptr;
    int rc = ba_create(ctx, p, &dev, /*transient*/ true);
    if (rc != OV2_OK) return rc;
    // chi2 / depth flags of inactive residual blocks keep the caller's values (the reference's removed
    // residual blocks keep their cached chi2err_): seed the device arrays with them
    rc = ba_run(ctx, dev, o, r, p->res_active ? r->chi2_last_eval : nullptr, p->res_active ? r->depthpos_last_eval : nullptr);
    ba_destroy(dev);
    return rc;
}

int ov2_ba_create(ov2_ctx *ctx, const ov2_ba_problem *p, ov2_ba_dev **out)
{
    OV2_REQUIRE(ctx && out, OV2_EINVAL, "NULL argument");
    *out = nullptr;
    return ba_create(ctx, p, out);
}

int ov2_ba_solve_resident(ov2_ctx *ctx, ov2_ba_dev *dev, const ov2_ba_options *o, ov2_ba_result *r)
{
    OV2_REQUIRE(ctx && dev, OV2_EINVAL, "NULL argument");
    return ba_run(ctx, dev, o, r, nullptr, nullptr);
}

void ov2_ba_destroy(ov2_ba_dev *dev) { ba_destroy(dev); }

void ov2_local_ba_default_options(ov2_local_ba_options *o)
{
    if (!o) return;
    o->robust_mono_th = 5.9915; o->use_robust_cost = 1; o->apply_l2_after_robust = 1; o->stop_requested = 0; o->stop_flag = nullptr;
    ov2_ba_default_options(&o->pass1);                       // 5 iterations, function_tolerance 1e-3 (optimizer.cpp:461-462)
    ov2_ba_default_options(&o->pass2);
    o->pass2.max_iter = 10;                                  // :611
}

// Optimizer::localBA's solve stage (src/optimizer.cpp:436-735) with the problem RESIDENT between the two passes: one
// counting sort + one upload, the outlier tests and the removal of residual blocks on the device, one download.
static int local_ba_one(ov2_ctx *ctx, const ov2_ba_problem *p, const ov2_local_ba_options *o, ov2_local_ba_result *r);
int ov2_local_ba(ov2_ctx *ctx, const ov2_ba_problem *p, const ov2_local_ba_options *o, ov2_local_ba_result *r)
{
    OV2_REQUIRE(ctx && p && o && r, OV2_EINVAL, "NULL argument");
    const int rc = local_ba_one(ctx, p, o, r);
    r->status = rc;
    return rc;
}
static int local_ba_one(ov2_ctx *ctx, const ov2_ba_problem *p, const ov2_local_ba_options *o, ov2_local_ba_result *r)
{
    OV2_REQUIRE(o->robust_mono_th > 0, OV2_EINVAL, "robust_mono_th must be positive");
    r->l2_done = 0; r->pass2_error = OV2_OK; r->n_bad_pass1 = 0; r->n_bad_total = 0;
    for (int i = 0; i < 2; i++) { r->iterations[i] = 0; r->num_successful_steps[i] = 0; r->termination[i] = OV2_TERM_NO_CONVERGENCE; r->initial_cost[i] = r->final_cost[i] = 0; r->solve_ms[i] = 0; }
    ov2_ba_dev *dev = nullptr;
    const bool dbg = ctx->debug != 0;
    const auto tw0 = std::chrono::steady_clock::now();
    auto lap = [&](const char *what) {
        if (dbg) fprintf(stderr, "[ov2 local_ba] %-28s %8.3f ms since entry\n", what, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tw0).count());
    };
    int rc = ba_create(ctx, p, &dev, /*transient*/ true);       // the pool lives in the context's scratch through both passes
    if (rc != OV2_OK) return rc;
    lap("sort + upload (ba_create)");
    struct Guard { ov2_ba_dev *d; ~Guard() { ba_destroy(d); } } guard{dev};
    if (dev->D.n_po > 0) { ov2_set_error("ov2_local_ba: problems with OV2_RES_PNP blocks go through ov2_ba_solve"); return OV2_EUNSUPPORTED; }
    BADev &D = dev->D;
    hipStream_t s = ctx->stream;
    const double huber = o->use_robust_cost ? sqrt(o->robust_mono_th) : -1.0;
    // pass 1 (:436-485)
    ov2_ba_options o1 = o->pass1;
    o1.huber_delta = huber;
    ov2_ba_result br;
    memset(&br, 0, sizeof(br));
    rc = ba_run(ctx, dev, &o1, &br, nullptr, nullptr);
    if (rc != OV2_OK) return rc;
    r->iterations[0] = br.iterations; r->num_successful_steps[0] = br.num_successful_steps; r->termination[0] = br.termination; r->initial_cost[0] = br.initial_cost;
    r->final_cost[0] = br.final_cost; r->solve_ms[0] = br.solve_ms;
    lap("pass 1");
    // outlier test on the values cached by the last Evaluate of pass 1 (:492-594)
    rc = ctx->reserve_host(64);
    if (rc != OV2_OK) return rc;
    int *cnt_h = (int *)ctx->h_scratch;
    const int mk_blocks = std::max(1, std::min(1024, (D.n_act + 255) / 256));
    hipLaunchKernelGGL(k_ba_mark_outliers, dim3(mk_blocks), dim3(256), 0, s, D, o->robust_mono_th, o->apply_l2_after_robust ? 1 : 0, (uint8_t *)nullptr);
    OV2_HIP_CHECK(hipGetLastError());
    OV2_HIP_CHECK(hipMemcpyAsync(cnt_h, D.lba_cnt, 16, hipMemcpyDeviceToHost, s));
    if (r->bad_after_pass1 && dev->n_res > 0) OV2_HIP_CHECK(hipMemcpyAsync(r->bad_after_pass1, D.bad_obs, (size_t)dev->n_res, hipMemcpyDeviceToHost, s));
    OV2_HIP_CHECK(hipStreamSynchronize(s));
    lap("outlier test 1");
    const int nbbad = cnt_h[0], left_remaining = cnt_h[1], right_remaining = cnt_h[2];
    r->n_bad_pass1 = nbbad; r->n_bad_total = nbbad;
    // stopLocalBA() is evaluated HERE, after the first solve (:603-604): a keyframe that arrived while pass 1 ran skips pass 2
    const bool stop = o->stop_requested || (o->stop_flag && *o->stop_flag);
    if (o->apply_l2_after_robust && o->use_robust_cost && !stop && nbbad > 0) {          // :603-604
        // the loss is reset to L2 only when both residual lists are still non-empty (:606-608: mono runs keep Huber!)
        ov2_ba_options o2 = o->pass2;
        o2.huber_delta = (left_remaining && right_remaining) ? -1.0 : huber;
        hipLaunchKernelGGL(k_ba_lm_live, dim3(std::max(1, std::min(512, (D.n_lm + 3) / 4))), dim3(256), 0, s, D);
        OV2_HIP_CHECK(hipMemsetAsync(D.lba_cnt, 0, 16, s));
        rc = ba_run(ctx, dev, &o2, &br, nullptr, nullptr, /*keep_state*/ true);
        if (rc != OV2_OK) {
            // pass 2 could not run: the device still holds an accepted state (pass 1's, or a later accepted LM step) and the
            // verdicts of the first test -- hand those back instead of dropping a valid solve
            r->pass2_error = rc;
            goto download;
        }
        r->l2_done = 1;
        r->iterations[1] = br.iterations; r->num_successful_steps[1] = br.num_successful_steps; r->termination[1] = br.termination; r->initial_cost[1] = br.initial_cost;
        r->final_cost[1] = br.final_cost; r->solve_ms[1] = br.solve_ms;
        lap("pass 2");
        // second outlier test on the residual blocks that are still in the problem (:637-735)
        hipLaunchKernelGGL(k_ba_mark_outliers, dim3(mk_blocks), dim3(256), 0, s, D, o->robust_mono_th, 0, (uint8_t *)nullptr);
        OV2_HIP_CHECK(hipGetLastError());
        OV2_HIP_CHECK(hipMemcpyAsync(cnt_h, D.lba_cnt, 16, hipMemcpyDeviceToHost, s));
    }
download:
    if (r->poses_out) OV2_HIP_CHECK(hipMemcpyAsync(r->poses_out, D.x_pose, 56 * (size_t)D.n_kf, hipMemcpyDeviceToHost, s));
    if (r->invdepth_out && D.n_lm > 0) OV2_HIP_CHECK(hipMemcpyAsync(r->invdepth_out, D.x_lam, 8 * (size_t)D.n_lm, hipMemcpyDeviceToHost, s));
    if (r->bad_obs && dev->n_res > 0) OV2_HIP_CHECK(hipMemcpyAsync(r->bad_obs, D.bad_obs, (size_t)dev->n_res, hipMemcpyDeviceToHost, s));
    if (r->chi2_last_eval && dev->n_res > 0) OV2_HIP_CHECK(hipMemcpyAsync(r->chi2_last_eval, D.chi2, 8 * (size_t)dev->n_res, hipMemcpyDeviceToHost, s));
    if (r->depthpos_last_eval && dev->n_res > 0) OV2_HIP_CHECK(hipMemcpyAsync(r->depthpos_last_eval, D.dpos, (size_t)dev->n_res, hipMemcpyDeviceToHost, s));
    OV2_HIP_CHECK(hipStreamSynchronize(s));
    if (r->l2_done) r->n_bad_total = nbbad + cnt_h[0];
    lap("outlier test 2 + download");
    return OV2_OK;
}

int ov2_local_ba_batch(ov2_ctx *ctx, int n, const ov2_ba_problem *p, const ov2_local_ba_options *o, ov2_local_ba_result *r, int *n_batched)
{
    if (n_batched) *n_batched = 0;
    OV2_REQUIRE(ctx && n >= 0 && (n == 0 || (p && o && r)), OV2_EINVAL, "NULL argument");
    if (n == 0) return OV2_OK;
    return local_ba_batch(ctx, n, p, o, r, n_batched);
}

int ov2_xyz_ba_solve(ov2_ctx *ctx, const ov2_xyzba_problem *p, const ov2_ba_options *o, ov2_xyzba_result *r)
{
    OV2_REQUIRE(ctx && p && o && r, OV2_EINVAL, "NULL argument");
    ov2_ba_dev *dev = nullptr;
    int rc = xyzba_create(ctx, p, &dev);
    if (rc != OV2_OK) return rc;
    ov2_ba_result br;
    memset(&br, 0, sizeof(br));
    br.poses_out = r->poses_out; br.invdepth_out = r->xyz_out; br.chi2_last_eval = r->chi2_last_eval; br.depthpos_last_eval = r->depthpos_last_eval;
    rc = ba_run(ctx, dev, o, &br, p->res_active ? r->chi2_last_eval : nullptr, p->res_active ? r->depthpos_last_eval : nullptr);
    ba_destroy(dev);
    r->iterations = br.iterations; r->num_successful_steps = br.num_successful_steps; r->initial_cost = br.initial_cost;
    r->final_cost = br.final_cost; r->termination = br.termination; r->solve_ms = br.solve_ms;
    return rc;
}

} // extern "C"
