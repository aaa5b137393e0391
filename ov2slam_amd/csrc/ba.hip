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
//
// Parts (one translation unit): ba_core.hpp -- the control block and the trust-region rules, shared with struct_ba.hip;
// ba_geom.hpp -- constants, the kernels' dynamic-LDS sizes, path choice and launch geometry (plain C++, the one owner of each);
// ba_chol.hpp -- the Cholesky kernels of the reduced system; ba_problem.hpp -- the device-resident problem (ba_create).
// This file: the kernels of the LM loop, the host LM driver (ba_lm_loop, ba_run, ba_run_batch), the localBA protocol.
#include "common.hpp"
#include <math.h>
#include <float.h>
#include <algorithm>
#include <stdlib.h>
#include <vector>
#include <functional>
#include <mutex>
#include <chrono>

#pragma clang fp contract(fast)   // BA parity is 1e-4 relative in fp64: FMA contraction is fine here
#include "ba_core.hpp"           // (after the pragma: the shared functions are compiled with contraction here)

#include "ba_geom.hpp"           // tile / panel constants, the kernels' dynamic-LDS sizes, path choice, launch geometry

#define BA_PART_MAX 2048
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
    // big = 1: more optimised keyframes than the LDS-resident path holds (69: ba_small_path).  W = E^T F is then kept SPARSE: one 6-double
    // "slot" per (landmark, optimised keyframe that sees or anchors it) in cww -- the anchor block and the left / right observer
    // blocks of one keyframe share a slot -- instead of a dense n_lm x nfp matrix.  The anchor-observer blocks of H go to HBM with
    // global atomics, the Schur complement is accumulated row block by row block in LDS from per-keyframe slot lists
    // (k_ba_schur_sparse) and the reduced system is factored by a multi-kernel blocked Cholesky on HBM (k_chol_*).
    int big, n_cw;
    int chol_hbm;                 // reduced system factored by the multi-kernel Cholesky on HBM (k_chol_*): always with big, and for 3-D point
                                  // problems (dense W, k_ba_schur_gemm) whose reduced system outgrows the one-work-group LDS kernel
    int lin_waves;                // 3-D point lineariser: wavefronts per work-group (each keeps 3 rows of W in LDS: ba_xyz_lin_waves)
    int lin_direct;               // big path with more optimised keyframes than the work-group's LDS can pre-aggregate (n_opt x 27 doubles:
                                  // ba_lin_direct): observer diagonal blocks and F^T b go to H / bf with global atomics as well
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

// ---------------------------------------------------------------------------------- algebra
#include "ba_pnp.hpp"            // d_se3_left_plus, d_residual_pnp: shared with pnp.hip

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
// dynamic LDS: 8*nfp (two W rows per wavefront) + n_opt*27 + 4*n_opt*21 + 4*LIN_RED doubles (lin_lds_bytes, ba_geom.hpp)
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

#include "ba_chol.hpp"          // the LDS-panel Cholesky (k_ba_cholesky) and the multi-kernel Cholesky on HBM (k_chol_*)

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
                const int valid = d_ctl_candidate(cl, O, ok, d_ctl_schur_model_cost_change(cl, P1, P2));
                if (valid) {
                    double d[6], out[7];
                    for (int c = 0; c < 6; c++) d[c] = -s_y[c] * s_scale[c];
                    d_se3_left_plus(xp, d, out);
                    for (int c = 0; c < 7; c++) cp[c] = out[c];
                    d_pose_to_RT(out, s_cRT);
                }
                s_flag = cl.done ? -1 : valid;                  // (an invalid step that used up the budget ends the solve)
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
        s_flag = d_ctl_candidate(cl, O, ok, d_ctl_schur_model_cost_change(cl, P1, P2));
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

#include "ba_problem.hpp"       // ov2_ba_dev, ba_create / xyzba_create / ba_destroy, the batch slices and the host thread pool

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

// ---------------------------------------------------------------------------------- host LM driver (single solve and lock-step batch)
static int ba_check_options(const ov2_ba_options *o)
{
    OV2_REQUIRE(o->max_iter >= 0 && o->initial_radius > 0 && o->min_lm_diagonal > 0 && o->min_lm_diagonal <= o->max_lm_diagonal,
                OV2_EINVAL, "bad solver options");
    return OV2_OK;
}

// Waits until the outcome of iteration `it` of all n problems is known: k_ba_decide stores 2 * iteration + done into each problem's
// pinned word (a finished problem reports `done` on its way out).  *all_done: every problem has terminated.
static int ba_wait_outcome(hipStream_t s, const volatile int *flag, int n, int it, bool *all_done)
{
    for (unsigned spins = 0;;) {
        int known = 0, done = 0;
        for (int i = 0; i < n; i++) { const int f = flag[i]; known += f >= 2 * it; done += f >= 0 && (f & 1); }
        *all_done = done == n;
        if (known == n) return OV2_OK;
#if !defined(__HIP_DEVICE_COMPILE__) && defined(__x86_64__)
        __builtin_ia32_pause();                                               // the estimator thread shares its core's siblings with the SLAM / mapper threads
#endif
        if ((++spins & 0x3FFFFFu) == 0) {                                 // (a watchdog, ~every 0.3 s: a query per wait put a 6 us bubble in front of the next launch)
            const hipError_t q = hipStreamQuery(s);
            if (q == hipSuccess) {                                    // everything enqueued has run: the words are final
                done = 0;
                for (int i = 0; i < n; i++) done += flag[i] >= 0 && (flag[i] & 1);
                *all_done = done == n;
                return OV2_OK;
            }
            if (q != hipErrorNotReady) OV2_HIP_CHECK(q);
        }
    }
}

// The LM loop, enqueued half an iteration ahead.  The first half of iteration `it` (bookkeeping, Schur complement, factorisation:
// ~265 us of config 4's ~385) goes into the stream BEFORE the outcome of iteration it - 1 is known; k_ba_decide stores that outcome
// into pinned host memory, and the second half (back-substitution .. decision, re-linearisation) follows when the host has seen
// it -- while the GPU is still busy with the first half, so the stream never drains.  A solve that converges pays four empty
// launches (every kernel starts with `if (ctl->done) return`): the two-iteration chunks of rounds 2-3 paid 18 plus a 4-byte
// device-to-host copy + event per chunk, a whole iteration of look-ahead 9.
// first_half(it), second_half(it): the caller's launches; bookkeeping(O): its k_ba_iter_begin launch outside an iteration.
template <class F1, class F2, class FB>
static int ba_lm_loop(hipStream_t s, const ov2_ba_options *o, const BAOpt &O, const volatile int *flag, int n, F1 first_half, F2 second_half, FB bookkeeping)
{
    const auto t_start = std::chrono::steady_clock::now();
    for (int it = 0; it < o->max_iter; it++) {
        if (it > 0 && o->max_solver_time_s > 0.0) {
            // Ceres tests total_time >= max_solver_time_in_seconds at the top of every iteration; here against the time the DEVICE
            // has actually spent (wait for the previous iteration first, otherwise only the enqueue is timed)
            OV2_HIP_CHECK(hipStreamSynchronize(s));
            if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count() >= o->max_solver_time_s) {
                // the regular per-iteration bookkeeping with an iteration budget of zero: it finalises the last step (successful
                // step count, minimum cost, cost of a fresh linearisation) and terminates with NO_CONVERGENCE
                BAOpt Ostop = O;
                Ostop.max_iter = 0;
                bookkeeping(Ostop);
                break;
            }
        }
        first_half(it);
        if (it >= 1) {
            bool all_done = false;
            const int rc = ba_wait_outcome(s, flag, n, it - 1, &all_done);
            if (rc != OV2_OK) return rc;
            if (all_done) break;
        }
        second_half(it);
    }
    bookkeeping(O);                                        // final bookkeeping
    OV2_HIP_CHECK(hipGetLastError());
    return OV2_OK;
}

static void ba_fill_result(ov2_ba_result *r, const BACtl &c, float ms)
{
    r->iterations = c.n_steps; r->num_successful_steps = c.n_success; r->termination = c.termination;
    r->initial_cost = c.initial_cost; r->final_cost = c.minimum_cost; r->solve_ms = ms;
}

// Dynamic-LDS limits are per-function, process-wide attributes: raised once to the hardware maximum (two contexts solving problems
// of different size on two threads would otherwise race on them).  The list is every kernel that is launched with dynamic LDS;
// what each asks for is its function in ba_geom.hpp.
static int ba_raise_lds_limits()
{
    static std::once_flag attr_once;
    static hipError_t attr_err = hipSuccess;
    std::call_once(attr_once, [] {
        const void *const fns[] = {
            (const void *)k_ba_linearize<false>, (const void *)k_chol_solve, (const void *)k_ba_linearize<true>,        // lin_lds_bytes, chol_solve_lds_bytes, lin_big_lds_bytes
            (const void *)k_ba_schur_sparse, (const void *)k_ba_linearize_xyz, (const void *)k_ba_cholesky,             // schur_sparse_lds_bytes, lin_xyz_lds_bytes, chol_lds_bytes
            (const void *)k_ba_linearize_po, (const void *)k_ba_linearize_B, (const void *)k_ba_cholesky_B,             // lin_po_lds_bytes, lin_lds_bytes, chol_lds_bytes
            (const void *)k_ba_backsub, (const void *)k_ba_backsub_xyz, (const void *)k_ba_backsub_B};                  // backsub_lds_bytes
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
        for (const void *fn : fns) if ((attr_err = raise(fn)) != hipSuccess) return;
    });
    OV2_HIP_CHECK(attr_err);
    return OV2_OK;
}

// What the host supplies to a fresh solve, before its clock starts.  one_reset: k_ba_reset copies the initial parameters and clears
// chi2 / depth flags on the device (b_ba_reset) -- only a caller's own seed of those two goes up; else everything is copied / set here
static int ba_upload_initial(hipStream_t s, const ov2_ba_dev *dev, bool one_reset, const double *chi2_init, const uint8_t *dpos_init)
{
    const BADev &D = dev->D;
    const size_t nr = (size_t)dev->n_res, nr1 = (size_t)std::max(1, dev->n_res);
    if (!one_reset) {
        OV2_HIP_CHECK(hipMemcpyAsync(D.x_pose, dev->h_poses0.data(), 56 * (size_t)D.n_kf, hipMemcpyHostToDevice, s));
        if (D.n_lm > 0) OV2_HIP_CHECK(hipMemcpyAsync(D.x_lam, dev->h_lam0.data(), 8 * (size_t)D.n_lm * D.ldim, hipMemcpyHostToDevice, s));
    }
    if (chi2_init) OV2_HIP_CHECK(hipMemcpyAsync(D.chi2, chi2_init, 8 * nr, hipMemcpyHostToDevice, s));
    else if (dpos_init || !one_reset) OV2_HIP_CHECK(hipMemsetAsync(D.chi2, 0xFF, 8 * nr1, s));       // NaN pattern: never evaluated
    if (dpos_init) OV2_HIP_CHECK(hipMemcpyAsync(D.dpos, dpos_init, nr, hipMemcpyHostToDevice, s));
    else if (chi2_init || !one_reset) OV2_HIP_CHECK(hipMemsetAsync(D.dpos, 0, nr1, s));
    return OV2_OK;
}

// the control block and the zeroed normal equations: one kernel (small inverse-depth problems, see b_ba_reset) or the round-1 sequence
static int ba_reset_system(hipStream_t s, const BADev &D, const BAGeom &G, const BACtl &h_ctl, bool one_reset, bool keep_state, bool host_chi2)
{
    if (one_reset) {
        hipLaunchKernelGGL(k_ba_reset, dim3(G.reset_blocks), dim3(256), 0, s, D, h_ctl, keep_state ? 1 : 0, host_chi2 ? 1 : 0);
        return OV2_OK;
    }
    OV2_HIP_CHECK(hipMemcpyAsync(D.ctl, &h_ctl, sizeof(h_ctl), hipMemcpyHostToDevice, s));
    OV2_HIP_CHECK(hipMemsetAsync(D.H, 0, 8 * (size_t)D.nfp * D.nfp, s));
    OV2_HIP_CHECK(hipMemsetAsync(D.bf, 0, 8 * (size_t)D.nfp, s));
    OV2_HIP_CHECK(hipMemsetAsync(D.yf, 0, 8 * (size_t)D.nfp, s));
    return OV2_OK;
}

// OV2_OPT_BA_DETERMINISTIC (BADev::det): one-wavefront lineariser work-groups with their own copies of H / F^T b / cost, one copy
// of W^T C W / v per landmark split; everything else of the solver is already a fixed-order computation.  The copies live in the
// CONTEXT (grow-only, like d_scratch): ov2_local_ba / ov2_ba_solve create a transient problem per call.  DG: k_ba_schur_gemm's view.
static int ba_det_setup(ov2_ctx *ctx, BADev &D, BADev &DG, const BAGeom &G)
{
    OV2_REQUIRE(D.ldim == 1 && !D.big, OV2_EUNSUPPORTED, "OV2_OPT_BA_DETERMINISTIC covers the inverse-depth form on the LDS-resident path only");
    hipStream_t s = ctx->stream;
    const size_t nn = (size_t)D.nfp * D.nfp, ncopy = (size_t)G.det_lin + G.det_po;
    const size_t b_H = up256(8 * ncopy * nn), b_bf = up256(8 * ncopy * D.nfp), b_c = up256(8 * std::max<size_t>(1, ncopy));
    const size_t b_G = up256(8 * (size_t)G.ksplit * nn), b_v = up256(8 * (size_t)G.ksplit * D.nfp);
    const size_t need = b_H + b_bf + b_c + b_G + b_v;
    if (need > ctx->ba_det_bytes) {
        if (ctx->ba_det_pool) { OV2_HIP_CHECK(hipStreamSynchronize(s)); (void)hipFree(ctx->ba_det_pool); ctx->ba_det_pool = nullptr; ctx->ba_det_bytes = 0; }
        hipError_t e = hipMalloc(&ctx->ba_det_pool, need);
        if (e != hipSuccess) { ov2_set_error("hipMalloc(%zu) for the deterministic mode: %s", need, hipGetErrorString(e)); return OV2_ENOMEM; }
        ctx->ba_det_bytes = need;
    }
    uint8_t *q = (uint8_t *)ctx->ba_det_pool;
    D.det = 1; D.det_lin = G.det_lin; D.det_po = G.det_po; D.det_ksplit = G.ksplit;
    D.Hpart = (double *)q; D.bfpart = (double *)(q + b_H); D.costpart = (double *)(q + b_H + b_bf);
    D.Gpart = (double *)(q + b_H + b_bf + b_c); D.vpart = (double *)(q + b_H + b_bf + b_c + b_G);
    OV2_HIP_CHECK(hipMemsetAsync(ctx->ba_det_pool, 0, b_H + b_bf + b_c, s));      // (the copies are clean between linearisations: k_ba_det_reduce clears as it reads)
    D.lin_blocks = G.det_lin;
    DG.det = 1; DG.det_ksplit = G.ksplit; DG.Gpart = D.Gpart; DG.vpart = D.vpart;
    return OV2_OK;
}

// the multi-kernel solve of one problem: state reset, first linearisation, the LM loop (D by value: the launches' view of the problem)
static int ba_enqueue_solve(ov2_ctx *ctx, const ov2_ba_dev *dev, BADev D, const BAGeom &G, const ov2_ba_options *o, const BAOpt &O,
                            const BACtl &h_ctl, bool one_reset, bool keep_state, bool host_chi2)
{
    hipStream_t s = ctx->stream;
    const int n_opt = D.nf / 6;
    int rc = ba_reset_system(s, D, G, h_ctl, one_reset, keep_state, host_chi2);
    if (rc != OV2_OK) return rc;
    // poses -> R | t, scales = 1 (round 1 filled the scales through a host staging vector: three copies and a synchronisation)
    hipLaunchKernelGGL(k_ba_init, dim3(G.init_blocks), dim3(256), 0, s, D);
    // rows of the W^T C W contraction: landmarks, or the 3 pseudo-rows per point of Wp (ldim 3)
    BADev DG = D;
    if (D.ldim == 3) { DG.W = D.Wp; DG.n_lm = 3 * D.n_lm; DG.cl = D.ones; DG.etb = D.ep; }
    if (ctx->ba_deterministic) {
        rc = ba_det_setup(ctx, D, DG, G);
        if (rc != OV2_OK) return rc;
    }

    auto linearize = [&]() {
        if (D.n_lm > 0 && D.ldim == 3) hipLaunchKernelGGL(k_ba_linearize_xyz, dim3(G.lin_blocks * (4 / D.lin_waves)), dim3(64 * D.lin_waves), G.lin_lds, s, D);
        else if (D.big) {
            // (k_ba_decide leaves H, F^T b and the W slots to this kernel on the large path: also for pose-only problems)
            if (D.n_lm > 0 || D.n_po > 0) hipLaunchKernelGGL(k_ba_zero_lin, dim3(1024), dim3(256), 0, s, D);
            if (D.n_lm > 0) hipLaunchKernelGGL(k_ba_linearize<true>, dim3(G.lin_blocks), dim3(256), G.lin_lds, s, D, dev->lm_order);
        }
        else if (D.det) {
            // one wavefront per work-group, each with its own copy of H / F^T b; then the copies in order
            if (D.n_lm > 0) hipLaunchKernelGGL(k_ba_linearize<false>, dim3(G.det_lin), dim3(64), G.lin_lds, s, D, dev->lm_order);
            if (D.n_po > 0) hipLaunchKernelGGL(k_ba_linearize_po, dim3(G.det_po), dim3(64), G.po_lds, s, D);
            hipLaunchKernelGGL(k_ba_det_reduce, dim3(256), dim3(256), 0, s, D);
            return;
        }
        else if (D.n_lm > 0) hipLaunchKernelGGL(k_ba_linearize<false>, dim3(G.lin_blocks), dim3(256), G.lin_lds, s, D, dev->lm_order);
        if (D.n_po > 0) hipLaunchKernelGGL(k_ba_linearize_po, dim3(G.po_blocks), dim3(256), G.po_lds, s, D);
    };
    linearize();
    if (!one_reset) OV2_HIP_CHECK(hipMemsetAsync(D.G, 0, 8 * (size_t)D.nfp * D.nfp, s));    // (every later iteration: cleared by the back-substitution kernel)
    rc = ctx->reserve_host(64);
    if (rc != OV2_OK) return rc;
    volatile int *flag_h = (volatile int *)ctx->h_scratch;
    flag_h[0] = -1;
    D.flag_h = (int *)ctx->h_scratch;
    DG.flag_h = D.flag_h;
    auto first_half = [&](int it) {
        hipLaunchKernelGGL(k_ba_iter_begin, dim3(1), dim3(1024), 0, s, D, O, it);
        if (D.ldim == 3 && D.n_lm > 0) hipLaunchKernelGGL(k_ba_xyz_prep, dim3(G.ws_blocks), dim3(256), 0, s, D);
        if (D.n_lm > 0 && D.big) hipLaunchKernelGGL(k_ba_schur_sparse, dim3(n_opt * G.ss_split, G.ss_chunks), dim3(64 * SS_WAVES), G.ss_lds, s, D, G.ss_split, G.ss_ncol);
        else if (D.n_lm > 0) hipLaunchKernelGGL(k_ba_schur_gemm, dim3(G.n_upper, G.ksplit), dim3(256), 0, s, DG, G.ntiles, G.lm_per_split);
        if (D.nf > 0) hipLaunchKernelGGL(k_ba_assemble, dim3((D.nf + 255) / 256, D.nf), dim3(256), 0, s, D);   // (structure-only problems: no reduced system)
        if (!D.chol_hbm) { hipLaunchKernelGGL(k_ba_cholesky, dim3(1), dim3(512), G.chol_lds, s, D); return; }
        for (int k0 = 0; k0 < D.nf; k0 += CH_NB) {
            const int m = D.nf - k0 - std::min(CH_NB, D.nf - k0);
            hipLaunchKernelGGL(k_chol_diag, dim3(1), dim3(64), 0, s, D, k0);
            if (m > 0) {
                const int mb = (m + 31) / 32;
                hipLaunchKernelGGL(k_chol_panel, dim3((m + 63) / 64), dim3(64), 0, s, D, k0);
                hipLaunchKernelGGL(k_chol_trail, dim3(mb * (mb + 1) / 2), dim3(256), 0, s, D, k0);
            }
        }
        hipLaunchKernelGGL(k_chol_solve, dim3(1), dim3(512), G.chol_lds, s, D);
    };
    auto second_half = [&](int it) {
        if (D.ldim == 3) hipLaunchKernelGGL(k_ba_backsub_xyz, dim3(G.ws_blocks), dim3(256), G.bs_lds, s, D);
        else hipLaunchKernelGGL(k_ba_backsub, dim3(G.bs_blocks), dim3(256), G.bs_lds, s, D);
        hipLaunchKernelGGL(k_ba_candidate, dim3(1), dim3(1024), 0, s, D, O);
        if (D.ldim == 3) hipLaunchKernelGGL(k_ba_cost_xyz, dim3(G.ws_blocks), dim3(256), 0, s, D);
        else hipLaunchKernelGGL(k_ba_cost, dim3(G.cost_blocks), dim3(256), 0, s, D);
        hipLaunchKernelGGL(k_ba_decide, dim3(1), dim3(1024), 0, s, D, O, it);
        linearize();
    };
    return ba_lm_loop(s, o, O, flag_h, 1, first_half, second_half,
                      [&](const BAOpt &Ob) { hipLaunchKernelGGL(k_ba_iter_begin, dim3(1), dim3(1024), 0, s, D, Ob, -1); });
}

// the result copies of a solve, asynchronous on s (a NULL destination is skipped)
static int ba_download(hipStream_t s, const ov2_ba_dev *dev, double *poses, double *lam, uint8_t *bad_obs, double *chi2, uint8_t *dpos)
{
    const BADev &D = dev->D;
    const size_t nr = (size_t)dev->n_res;
    if (poses) OV2_HIP_CHECK(hipMemcpyAsync(poses, D.x_pose, 56 * (size_t)D.n_kf, hipMemcpyDeviceToHost, s));
    if (lam && D.n_lm > 0) OV2_HIP_CHECK(hipMemcpyAsync(lam, D.x_lam, 8 * (size_t)D.n_lm * D.ldim, hipMemcpyDeviceToHost, s));
    if (bad_obs && nr > 0) OV2_HIP_CHECK(hipMemcpyAsync(bad_obs, D.bad_obs, nr, hipMemcpyDeviceToHost, s));
    if (chi2 && nr > 0) OV2_HIP_CHECK(hipMemcpyAsync(chi2, D.chi2, 8 * nr, hipMemcpyDeviceToHost, s));
    if (dpos && nr > 0) OV2_HIP_CHECK(hipMemcpyAsync(dpos, D.dpos, nr, hipMemcpyDeviceToHost, s));
    return OV2_OK;
}

// what a solve adds to the launches' view of a problem: the loss, the clamp of the LM diagonal, and the grids whose per-work-group
// partial sums the bookkeeping kernels add up (G: the launches' geometry -- the problem's own, or its batch's)
static void ba_view_for_solve(BADev &D, const ov2_ba_options *o, double huber, const BAGeom &G)
{
    D.huber = huber; D.min_diag = o->min_lm_diagonal; D.max_diag = o->max_lm_diagonal;
    D.bs_blocks = G.bs_blocks; D.cost_blocks = G.cost_blocks; D.lin_blocks = G.lin_blocks;
}

// keep_state: continue from the parameters and the cached chi2 / depth flags that are on the device (second pass of
// ov2_local_ba) instead of resetting to the problem's initial values
static int ba_run(ov2_ctx *ctx, ov2_ba_dev *dev, const ov2_ba_options *o, ov2_ba_result *r,
                  const double *chi2_init, const uint8_t *dpos_init, bool keep_state = false)
{
    OV2_REQUIRE(o && r, OV2_EINVAL, "NULL options/result");
    int rc = ba_check_options(o);
    if (rc != OV2_OK) return rc;
    OV2_HIP_CHECK(hipSetDevice(ctx->device));
    BADev D = dev->D;
    hipStream_t s = ctx->stream;
    const BAOpt O = ba_opt_from(*o);
    // a problem alone spreads over the whole chip: up to 256 lineariser work-groups, ~1024 for the Schur complement
    const BAGeom G = ba_geom(D, 256, 1024, ctx->ba_schur_chunk);
    ba_view_for_solve(D, o, o->huber_delta, G);
    // size limits first: nothing is created or enqueued for a problem this path cannot solve
    OV2_REQUIRE(G.lin_lds <= BA_LIN_LDS_MAX, OV2_EUNSUPPORTED, "too many optimised keyframes for the LDS-aggregating lineariser");
    OV2_REQUIRE(G.chol_lds <= BA_CHOL_LDS_MAX, OV2_EUNSUPPORTED, "reduced system too large for the LDS-panel Cholesky");
    rc = ba_raise_lds_limits();
    if (rc == OV2_OK) rc = ba_events(ctx);
    if (rc != OV2_OK) return rc;
    // one optimised pose, pose-only residual blocks, no landmarks (ceresPnP): the whole loop in one kernel (OV2_OPT_BA_POSE_ONLY_FUSED
    // = 0 keeps the multi-kernel path for A/B runs)
    const bool fused_po = D.n_lm == 0 && D.n_po > 0 && D.nf == 6 && D.ldim == 1 && ctx->ba_pose_only_fused && !(o->max_solver_time_s > 0.0) && !ctx->ba_deterministic;
    // small inverse-depth problems: one reset kernel instead of copies and memsets; pose-only fused solves and the other forms keep the round-1 sequence
    const bool one_reset = D.ldim == 1 && !D.big && D.pose0 != nullptr && !fused_po;
    if (!keep_state) {
        rc = ba_upload_initial(s, dev, one_reset, chi2_init, dpos_init);
        if (rc != OV2_OK) return rc;
    }
    OV2_HIP_CHECK(hipEventRecord(ctx->ba_ev[0], s));
    BAIterRec *trace = nullptr;
    rc = ba_trace_begin(ctx, ctx->ba_trace != 0, &trace);
    if (rc != OV2_OK) return rc;
    BACtl h_ctl;
    ba_ctl_init(h_ctl, o->initial_radius, trace);
    if (fused_po) {
        hipLaunchKernelGGL(k_ba_pose_only, dim3(1), dim3(256), 0, s, D, O, h_ctl);
        OV2_HIP_CHECK(hipGetLastError());
    } else {
        rc = ba_enqueue_solve(ctx, dev, D, G, o, O, h_ctl, one_reset, keep_state, chi2_init || dpos_init);
        if (rc != OV2_OK) return rc;
    }
    OV2_HIP_CHECK(hipEventRecord(ctx->ba_ev[1], s));
    OV2_HIP_CHECK(hipMemcpyAsync(&h_ctl, D.ctl, sizeof(h_ctl), hipMemcpyDeviceToHost, s));
    rc = ba_download(s, dev, r->poses_out, r->invdepth_out, nullptr, r->chi2_last_eval, r->depthpos_last_eval);
    if (rc != OV2_OK) return rc;
    OV2_HIP_CHECK(hipStreamSynchronize(s));
    if (h_ctl.trace) {
        rc = ba_trace_fetch(ctx, h_ctl.n_trace);
        if (rc != OV2_OK) return rc;
    }
    float ms = 0;
    OV2_HIP_CHECK(hipEventElapsedTime(&ms, ctx->ba_ev[0], ctx->ba_ev[1]));
    ba_fill_result(r, h_ctl, ms);
    if (ctx->debug)
        fprintf(stderr, "[ov2 ba] cholesky ticks (100MHz): copy-in %llu pivot+panel %llu write-back %llu trailing %llu block inverses %llu solves %llu\n",
                h_ctl.dbg[0], h_ctl.dbg[1], h_ctl.dbg[2], h_ctl.dbg[3], h_ctl.dbg[4], h_ctl.dbg[5]);
    return OV2_OK;
}

#include "ba_local.hpp"         // the two-pass localBA protocol: one problem (local_ba_one), a lock-step batch (local_ba_batch)

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

int ov2_local_ba(ov2_ctx *ctx, const ov2_ba_problem *p, const ov2_local_ba_options *o, ov2_local_ba_result *r)
{
    OV2_REQUIRE(ctx && p && o && r, OV2_EINVAL, "NULL argument");
    const int rc = local_ba_one(ctx, p, o, r);
    r->status = rc;
    return rc;
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
