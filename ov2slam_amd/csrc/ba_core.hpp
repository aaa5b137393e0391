// ba_core.hpp -- what every device bundle-adjustment solver shares: Ceres' trust-region Levenberg-Marquardt rules as functions
// on the control block (BACtl), and the small algebra around them.  Included by ba.hip (the multi-kernel solver and the
// one-kernel pose-only solver) and struct_ba.hip (the one-kernel structure-only solver).
//
// Floating point: nothing here sets a contraction mode.  Each file includes this header AFTER its own file-scope
// `#pragma clang fp contract(...)`, which then governs these functions too (ba.hip: fast, struct_ba.hip: off).
#pragma once
#include "common.hpp"
#include <math.h>
#include <float.h>
#include <stdlib.h>

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

struct BAOpt {
    int max_iter;
    double ftol, gtol, ptol, max_radius, min_radius, min_diag, max_diag, min_rel_decrease;
    int jacobi, max_invalid;
};

static inline BAOpt ba_opt_from(const ov2_ba_options &o)
{
    BAOpt O;
    O.max_iter = o.max_iter; O.ftol = o.function_tolerance; O.gtol = o.gradient_tolerance; O.ptol = o.parameter_tolerance;
    O.max_radius = o.max_radius; O.min_radius = o.min_radius; O.min_diag = o.min_lm_diagonal; O.max_diag = o.max_lm_diagonal;
    O.min_rel_decrease = o.min_relative_decrease; O.jacobi = o.jacobi_scaling; O.max_invalid = o.max_consecutive_invalid_steps;
    return O;
}

// the control block before iteration zero: a linearisation is wanted, "the last step was successful" (so that iteration
// zero counts as one, trust_region_minimizer.cc IterationZero), no parameter norm yet
__host__ __device__ inline void ba_ctl_init(BACtl &c, double initial_radius, BAIterRec *trace)
{
    c = BACtl{};
    c.radius = initial_radius; c.decrease_factor = 2.0; c.x_norm = -1.0;
    c.need_lin = 1; c.step_successful = 1;
    c.termination = OV2_TERM_NO_CONVERGENCE;
    c.cur.gradient_norm = NAN;                              // (the device forms the max norm only)
    c.trace = trace;
}

// ---------------------------------------------------------------------------------- host scaffolding of a solve
// the context's two timing events (ov2_ctx::ba_ev), created with the first solve and destroyed with the context: a pair per
// pass was 25 us
static inline int ba_events(ov2_ctx *ctx)
{
    for (int i = 0; i < 2; i++) if (!ctx->ba_ev[i]) OV2_HIP_CHECK(hipEventCreate(&ctx->ba_ev[i]));
    return OV2_OK;
}

// OV2_OPT_BA_TRACE.  Begin: no record yet; on: the buffers exist (allocated with the first traced solve) and *trace is the
// device one for the control block, else NULL.  Fetch (after the solve's synchronisation): the n_trace records the device wrote.
static inline int ba_trace_begin(ov2_ctx *ctx, bool on, BAIterRec **trace)
{
    ctx->ba_trace_n = 0;
    *trace = nullptr;
    if (!on) return OV2_OK;
    if (!ctx->ba_trace_d) OV2_HIP_CHECK(hipMalloc(&ctx->ba_trace_d, sizeof(BAIterRec) * BA_TRACE_CAP));
    if (!ctx->ba_trace_h) { ctx->ba_trace_h = malloc(sizeof(BAIterRec) * BA_TRACE_CAP); OV2_REQUIRE(ctx->ba_trace_h, OV2_ENOMEM, "trace buffer"); }
    *trace = (BAIterRec *)ctx->ba_trace_d;
    return OV2_OK;
}
static inline int ba_trace_fetch(ov2_ctx *ctx, int n_trace)
{
    ctx->ba_trace_n = n_trace;
    const int nrec = n_trace < BA_TRACE_CAP ? n_trace : BA_TRACE_CAP;
    if (nrec > 0) OV2_HIP_CHECK(hipMemcpy(ctx->ba_trace_h, ctx->ba_trace_d, sizeof(BAIterRec) * (size_t)nrec, hipMemcpyDeviceToHost));
    return OV2_OK;
}

// ---------------------------------------------------------------------------------- trust-region bookkeeping (one thread)
// The three scalar state machines of Ceres' TrustRegionMinimizer as pure functions on the control block, shared by the
// multi-kernel solver (k_ba_iter_begin / k_ba_candidate / k_ba_decide) and the single-kernel solvers (k_ba_pose_only,
// k_structure_ba): there the block sits in LDS, one thread makes the call between two barriers and all threads read the verdict.
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

// model_cost_change = -(J step).(r + J step / 2) with step = -y  ==  y.g' - y^T H' y / 2, from the Schur-form partial sums:
// P1 = y . g'_f, P2 = y^T H'_pp y of the pose part, the landmark part in the control block's accumulators
__device__ __forceinline__ double d_ctl_schur_model_cost_change(const BACtl &cl, double P1, double P2)
{
    return (P1 + cl.acc1) - 0.5 * (P2 + cl.acc3 + cl.acc2);
}

// judges the step: returns 1 when it is valid (ok: the linear solve gave a finite step; model cost change mcc > 0)
__device__ __forceinline__ int d_ctl_candidate(BACtl &cl, const BAOpt &O, int ok, double mcc)
{
    BACtl *ctl = &cl;
    int valid = 0;
    if (ok) {
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
// unit quaternion (x, y, z, w; normalised here) -> rotation matrix, row-major
__host__ __device__ __forceinline__ void d_quat_to_R(const double *q, double *R)
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

// ---------------------------------------------------------------------------------- reductions
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
