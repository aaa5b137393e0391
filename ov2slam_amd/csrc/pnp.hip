// pnp.hip -- the per-frame pose on gfx950 (fp64): MultiViewGeometry::ceresPnP's whole two-pass protocol in ONE kernel
// (src/multi_view_geometry.cpp:492-586) and VisualFrontEnd::computePose as one device-resident chain
// (src/visual_front_end.cpp:659-851), single and batched with the problem as a grid axis.
//   k_pnp_solve    ONE WORK-GROUP PER PROBLEM (blockIdx.x = item): pass 1 (Huber), the outlier test on the values of the last
//                  Evaluate, pass 2 (L2 over the remaining blocks, a fresh control block), the ascending outlier list.  The
//                  trust-region rules are the functions k_ba_pose_only calls (ba_core.hpp, ba_pnp.hpp); that kernel is untouched.
//                  Sums over the blocks are formed in a FIXED order (lane partials in block order with stride PNP_THREADS,
//                  wave_sum, one LDS slot per wavefront and value, thread 0 adds the slots in wavefront order): no atomics, so a
//                  problem gives the same bits in every run, at every position of a batch, and inside the chain.
//   k_pose_gather  one wavefront per item, after the P3P search (p3p_dev.hpp): judges P3P's result, turns its model into the pose
//                  PnP starts from, and compacts unpx / wpt / sigma past P3P's outliers (stable, ballot prefix).
//   k_pose_decide  one wavefront per item, after k_pnp_solve: the acceptance test, the action, the removal bytes.
// Every loop is bounded by an argument (n, max_iter, n_outliers <= n); no work-group waits on another; every index is below the
// item's point count by construction (P3P's outlier indices are checked against it all the same).
#include "common.hpp"
#include "p3p_dev.hpp"
#include "mvg_dev.hpp"                // pose_from_model (epifilter.hip builds the mono pose from it too)
#include "pose_dev.hpp"               // PnPItem, PnPOut, PoseItem, PoseOut; the chain as host steps (trackb.hip runs it too)
#include <cmath>
#include <cfloat>
#include <vector>

#pragma clang fp contract(fast)   // as ba.hip: the shared trust-region functions are compiled with contraction here too
#include "ba_core.hpp"
#include "ba_pnp.hpp"

// One size for every form (single, batch, chain): the bits of a problem depend on it.  Measured on the MI355X.
#ifndef PNP_THREADS
#define PNP_THREADS 128
#endif
#define PNP_WAVES (PNP_THREADS / 64)
#define PNP_MAX_POINTS OV2_P3P_MAX_POINTS
static_assert(PNP_THREADS == 64 || PNP_THREADS == 128 || PNP_THREADS == 256, "PNP_THREADS");

struct PnPArgs {
    const PnPItem *items;
    const double *unpx, *wpt, *sigma;      // 2, 3, 1 per block, item b's at items[b].pt0
    const double *pose0;                   // 7 per item
    PnPOut *out; int *outliers;            // the outlier list of item b at items[b].pt0
    double calib_l[4];                     // (the name d_residual_pnp reads)
    double huber, chi2th, initial_radius;
    int apply_l2;
    BAOpt O;
};

__global__ __launch_bounds__(PNP_THREADS) void k_pnp_solve(PnPArgs a)
{
    __shared__ BACtl cl;
    __shared__ double s_H[21], s_b[6], s_cost, s_part[PNP_WAVES][28], s_scale[6], s_diag[6], s_y[6];
    __shared__ double s_x[7], s_xRT[12], s_c[7], s_cRT[12];      // the pose and its candidate (+ cached R | t)
    __shared__ double s_L[6][6], s_t[6];                         // thread 0's 6 x 6 factor and right-hand side (private arrays with a
                                                                 // run-time index would live in scratch)
    __shared__ int s_flag, s_nbad;
    __shared__ uint8_t s_bad[PNP_MAX_POINTS];                    // pass 1: the outlier test of the last Evaluate; pass 2: the removed blocks
    const PnPItem item = a.items[blockIdx.x];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = item.n;
    const BAOpt O = a.O;
    PnPOut &out = a.out[blockIdx.x];
    const double *unpx = a.unpx + 2 * (size_t)item.pt0, *wpt = a.wpt + 3 * (size_t)item.pt0, *sigma = a.sigma + item.pt0;
    if (tid == 0) {
        for (int c = 0; c < 7; c++) s_x[c] = a.pose0[7 * (size_t)blockIdx.x + c];
        d_pose_to_RT(s_x, s_xRT);
        for (int q = 0; q < 2; q++) { out.ran[q] = 0; out.iterations[q] = 0; out.n_success[q] = 0; out.termination[q] = 0; out.initial_cost[q] = 0; out.final_cost[q] = 0; }
        out.success = 0; out.n_out = 0;
    }
    if (n <= 0 || n > PNP_MAX_POINTS) {                          // (uniform) an empty item: "every block is bad", nothing ran
        if (tid == 0) for (int c = 0; c < 7; c++) out.pose[c] = s_x[c];
        return;
    }
    auto Hd = [&](int i, int j) { const int p = i < j ? i : j, q = i < j ? j : i; return s_H[p * 6 - p * (p - 1) / 2 + (q - p)]; };   // upper-packed

    int last_term = OV2_TERM_FAILURE;
    for (int pass = 0; pass < 2; pass++) {
        const double huber = pass == 0 ? a.huber : -1.0;
        if (tid == 0) ba_ctl_init(cl, a.initial_radius, nullptr);
        if (tid < 6) { s_scale[tid] = 1.0; s_diag[tid] = 0.0; s_y[tid] = 0.0; }
        __syncthreads();

        // J^T J (upper triangle, 21), J^T r (6) and the robustified cost at x, in a fixed order
        auto linearize = [&]() {
            double v[28];
            for (int q = 0; q < 28; q++) v[q] = 0;
            for (int k = tid; k < n; k += PNP_THREADS) {
                if (pass && s_bad[k]) continue;
                double r[2], Jo[12];
                const int dp = d_residual_pnp<true>(a, s_xRT, wpt + 3 * k, unpx + 2 * k, sigma[k], r, Jo);
                const double sq = r[0] * r[0] + r[1] * r[1];
                if (!pass) s_bad[k] = (uint8_t)(sq > a.chi2th || !dp);
                double rho0, rho1;
                d_huber(huber, sq, rho0, rho1);
                v[27] += 0.5 * rho0;
                const double sc = sqrt(rho1);
                r[0] *= sc; r[1] *= sc;
                for (int q = 0; q < 12; q++) Jo[q] *= sc;
                int t = 0;
                for (int c = 0; c < 6; c++) {
                    v[21 + c] += Jo[c] * r[0] + Jo[6 + c] * r[1];
                    for (int d = c; d < 6; d++) v[t++] += Jo[c] * Jo[d] + Jo[6 + c] * Jo[6 + d];
                }
            }
            for (int q = 0; q < 28; q++) { const double t = wave_sum(v[q]); if (lane == 0) s_part[wave][q] = t; }
            __syncthreads();
            if (tid == 0) {
                for (int q = 0; q < 28; q++) {
                    double t = s_part[0][q];
                    for (int w = 1; w < PNP_WAVES; w++) t += s_part[w][q];
                    if (q < 21) s_H[q] = t; else if (q < 27) s_b[q - 21] = t; else s_cost = t;
                }
                cl.cost_acc += s_cost; cl.need_lin = 0; cl.fresh_lin = 1;      // (a linearisation at x is now available)
            }
            __syncthreads();
        };

        linearize();
        for (int it = 0; it <= O.max_iter; it++) {
            // ---- iteration bookkeeping, the 6 x 6 solve and the candidate (as k_ba_pose_only) ----
            if (tid == 0) {
                const int fresh = cl.fresh_lin;
                double gm = 0;
                if (fresh) {
                    if (O.jacobi && !cl.scaled) for (int c = 0; c < 6; c++) s_scale[c] = 1.0 / (1.0 + sqrt(Hd(c, c)));
                    double d[6], o7[7];
                    for (int c = 0; c < 6; c++) d[c] = -s_b[c];
                    d_se3_left_plus(s_x, d, o7);
                    for (int c = 0; c < 7; c++) gm = fmax(gm, fabs(s_x[c] - o7[c]));
                }
                d_ctl_iter_begin(cl, O, fresh, gm);
                if (!cl.done) {
                    if (!cl.reuse_diag) for (int c = 0; c < 6; c++) s_diag[c] = fmin(fmax(s_scale[c] * s_scale[c] * Hd(c, c), O.min_diag), O.max_diag);
                    cl.reuse_diag = 1;
                    double (*L)[6] = s_L, *y = s_t;
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
                        double d[6], o7[7];
                        for (int c = 0; c < 6; c++) d[c] = -s_y[c] * s_scale[c];
                        d_se3_left_plus(s_x, d, o7);
                        for (int c = 0; c < 7; c++) s_c[c] = o7[c];
                        d_pose_to_RT(o7, s_cRT);
                    }
                    s_flag = cl.done ? -1 : valid;              // (an invalid step that used up the budget ends the solve)
                } else s_flag = -1;
            }
            __syncthreads();
            const int f1 = s_flag;
            if (f1 < 0) break;                                      // terminated in the bookkeeping
            if (f1 == 0) { __syncthreads(); continue; }             // invalid step: radius already shrunk, same linearisation
            // ---- the cost at the candidate (also the values the outlier test reads, N4) ----
            double cost = 0;
            for (int k = tid; k < n; k += PNP_THREADS) {
                if (pass && s_bad[k]) continue;
                double r[2];
                const int dp = d_residual_pnp<false>(a, s_cRT, wpt + 3 * k, unpx + 2 * k, sigma[k], r, nullptr);
                const double sq = r[0] * r[0] + r[1] * r[1];
                if (!pass) s_bad[k] = (uint8_t)(sq > a.chi2th || !dp);
                double rho0, rho1;
                d_huber(huber, sq, rho0, rho1);
                cost += 0.5 * rho0;
            }
            cost = wave_sum(cost);
            if (lane == 0) s_part[wave][27] = cost;
            __syncthreads();
            // ---- accept or reject ----
            if (tid == 0) {
                double t = s_part[0][27];
                for (int w = 1; w < PNP_WAVES; w++) t += s_part[w][27];
                cl.cost_acc += t;
                double SN = 0, XN = 0;
                for (int c = 0; c < 7; c++) { const double d = s_x[c] - s_c[c]; SN += d * d; XN += s_c[c] * s_c[c]; }
                const int accept = d_ctl_decide(cl, O, SN, XN);
                if (accept) { for (int c = 0; c < 7; c++) s_x[c] = s_c[c]; for (int c = 0; c < 12; c++) s_xRT[c] = s_cRT[c]; }
                s_flag = cl.done ? -1 : (cl.need_lin ? 1 : 0);
            }
            __syncthreads();
            const int f2 = s_flag;
            if (f2 < 0) break;
            if (f2 == 1) linearize(); else __syncthreads();         // (s_flag is rewritten only after every thread has read it)
        }
        __syncthreads();
        if (tid == 0) {
            out.ran[pass] = 1; out.iterations[pass] = cl.n_steps; out.n_success[pass] = cl.n_success; out.termination[pass] = cl.termination;
            out.initial_cost[pass] = cl.initial_cost; out.final_cost[pass] = cl.minimum_cost;
        }
        last_term = cl.termination;
        if (pass == 1) break;
        // ---- the outlier test of pass 1, ascending, by the first wavefront ----
        if (wave == 0) {
            int nb = 0;
            int *ol = a.outliers + item.pt0;
            for (int i0 = 0; i0 < n; i0 += 64) {
                const int i = i0 + lane;
                const bool bad = i < n && s_bad[i];
                const unsigned long long m = __ballot(bad);
                if (bad) ol[nb + __popcll(m & ((1ull << lane) - 1ull))] = i;
                nb += __popcll(m);
            }
            if (lane == 0) s_nbad = nb;
        }
        __syncthreads();
        const int nbad = s_nbad;
        if (tid == 0) out.n_out = nbad;
        if (nbad == n) { last_term = OV2_TERM_FAILURE; break; }     // every block is bad: false, with the pose of pass 1
        if (!(a.apply_l2 && nbad > 0)) break;
    }
    if (tid == 0) {
        out.success = last_term <= OV2_TERM_MIN_RADIUS;             // Summary::IsSolutionUsable
        for (int c = 0; c < 7; c++) out.pose[c] = s_x[c];
    }
}

// ================================================================================== the chain around it
#pragma clang fp contract(off)    // from here on every expression rounds as written (the host form of pose_from_model must agree)

enum { POSE_ST_TOO_FEW = 0, POSE_ST_P3P_FAIL = 1, POSE_ST_PNP = 2, POSE_ST_P3P_PNP = 3 };   // what k_pose_gather found

struct PoseArgs {
    const PoseItem *items;
    const double *Twc, *unpx, *wpt, *sigma;            // the caller's arrays (7 per item; 2, 3, 1 per point)
    const P3Item *p3items; const P3Out *p3out; const int *p3ol;   // the search's items, results and outlier lists (NULL: no item searched)
    double *c_unpx, *c_wpt, *c_sigma; int *idx;        // what PnP reads: the remaining points and their indices in the caller's arrays
    PnPItem *pnp_items; double *pose0; int *stage;
    const PnPOut *pnp_out; const int *pnp_ol;
    PoseOut *out; uint8_t *removed;
    int mono;
};

__global__ __launch_bounds__(64) void k_pose_gather(PoseArgs a)
{
    __shared__ uint8_t s_rm[PNP_MAX_POINTS];
    const int b = blockIdx.x, lane = threadIdx.x;
    const PoseItem it = a.items[b];
    const int n = it.n;
    const size_t p0 = (size_t)it.pt0;
    int stage, m = 0;
    double pose[7];
    for (int c = 0; c < 7; c++) pose[c] = a.Twc[7 * (size_t)b + c];
    for (int i = lane; i < n; i += 64) s_rm[i] = 0;
    if (n < 4) stage = POSE_ST_TOO_FEW;
    else if (it.do_p3p) {
        const P3Out &o = a.p3out[b];
        const bool fail = o.status != 0 || o.n_inliers < 5 || !isfinite(o.model[9]) || !isfinite(o.model[10]) || !isfinite(o.model[11]);
        if (fail) stage = POSE_ST_P3P_FAIL;
        else {
            stage = POSE_ST_P3P_PNP;
            pose_from_model(o.model, pose);
            const int *ol = a.p3ol + a.p3items[b].pt0;
            const int no = o.n_outliers < n ? o.n_outliers : n;
            __syncthreads();
            for (int k = lane; k < no; k += 64) { const int i = ol[k]; if (i >= 0 && i < n) s_rm[i] = 1; }
        }
    } else stage = POSE_ST_PNP;
    __syncthreads();
    if (stage >= POSE_ST_PNP) {
        for (int i0 = 0; i0 < n; i0 += 64) {
            const int i = i0 + lane;
            const bool keep = i < n && !s_rm[i];
            const unsigned long long mk = __ballot(keep);
            if (keep) {
                const size_t d = p0 + (size_t)(m + __popcll(mk & ((1ull << lane) - 1ull))), s = p0 + (size_t)i;
                a.c_unpx[2 * d] = a.unpx[2 * s]; a.c_unpx[2 * d + 1] = a.unpx[2 * s + 1];
                a.c_wpt[3 * d] = a.wpt[3 * s]; a.c_wpt[3 * d + 1] = a.wpt[3 * s + 1]; a.c_wpt[3 * d + 2] = a.wpt[3 * s + 2];
                a.c_sigma[d] = a.sigma[s];
                a.idx[d] = i;
            }
            m += __popcll(mk);
        }
    }
    for (int i = lane; i < n; i += 64) a.removed[p0 + i] = stage == POSE_ST_P3P_PNP ? s_rm[i] : 0;
    if (lane == 0) {
        a.pnp_items[b] = PnPItem{m, it.pt0, 0, 0};
        for (int c = 0; c < 7; c++) a.pose0[7 * (size_t)b + c] = pose[c];
        a.stage[b] = stage;
    }
}

__global__ __launch_bounds__(64) void k_pose_decide(PoseArgs a)
{
    const int b = blockIdx.x, lane = threadIdx.x;
    const PoseItem it = a.items[b];
    const int stage = a.stage[b], m = a.pnp_items[b].n;
    const size_t p0 = (size_t)it.pt0;
    const PnPOut &r = a.pnp_out[b];
    int action, req = it.p3p_req;
    const double *pose = a.Twc + 7 * (size_t)b;
    const bool searched = stage == POSE_ST_P3P_FAIL || stage == POSE_ST_P3P_PNP;
    if (stage == POSE_ST_TOO_FEW) action = OV2_POSE_TOO_FEW;
    else if (stage == POSE_ST_P3P_FAIL) action = OV2_POSE_P3P_RESET;
    else {
        const bool reject = !r.success || m - r.n_out < 5 || (double)r.n_out > 0.5 * (double)m ||
                            !isfinite(r.pose[0]) || !isfinite(r.pose[1]) || !isfinite(r.pose[2]);
        if (!reject) {
            action = OV2_POSE_OK; req = 0; pose = r.pose;
            const int *ol = a.pnp_ol + p0;
            for (int k = lane; k < r.n_out && k < m; k += 64) { const int j = ol[k]; if (j >= 0 && j < m) a.removed[p0 + a.idx[p0 + j]] = 2; }
        } else if (stage == POSE_ST_PNP) { action = OV2_POSE_PNP_REQ_P3P; req = 1; }
        else { action = a.mono ? OV2_POSE_PNP_RESET : OV2_POSE_PNP_KEEP; pose = a.pose0 + 7 * (size_t)b; }
    }
    if (lane == 0) {
        PoseOut &o = a.out[b];
        for (int c = 0; c < 7; c++) o.Twc[c] = pose[c];
        o.action = action; o.p3p_req_out = req;
        o.n_removed_p3p = stage == POSE_ST_P3P_PNP ? it.n - m : 0;
        o.n_outliers_pnp = stage >= POSE_ST_PNP ? r.n_out : 0;
        o.ran_p3p = searched;
        if (searched) {
            const P3Out &p = a.p3out[b];
            o.p3p_status = p.status; o.p3p_best_row = p.best_row; o.p3p_iterations = p.iterations; o.p3p_rows_consumed = p.rows_consumed; o.p3p_score = p.score;
        } else { o.p3p_status = 0; o.p3p_best_row = -1; o.p3p_iterations = 0; o.p3p_rows_consumed = 0; o.p3p_score = 0.0; }
        for (int q = 0; q < 2; q++) {
            o.ran[q] = r.ran[q]; o.iterations[q] = r.iterations[q]; o.n_success[q] = r.n_success[q]; o.termination[q] = r.termination[q];
            o.initial_cost[q] = r.initial_cost[q]; o.final_cost[q] = r.final_cost[q];
        }
        o.pad = 0;
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------
static int pnp_check_params(const ov2_pnp_params *p)
{
    OV2_REQUIRE(p, OV2_EINVAL, "NULL params");
    OV2_REQUIRE(p->nmaxiter >= 0, OV2_EINVAL, "nmaxiter < 0");
    OV2_REQUIRE(std::isfinite(p->chi2th) && p->chi2th > 0.0, OV2_EINVAL, "chi2th <= 0 or not finite");
    for (int c = 0; c < 4; c++) OV2_REQUIRE(std::isfinite(p->K[c]), OV2_EINVAL, "K not finite");
    OV2_REQUIRE(p->K[0] != 0.0 && p->K[1] != 0.0, OV2_EINVAL, "fx / fy == 0");
    return OV2_OK;
}

// the arrays of one problem (the pose problem has the same leading members)
static int pnp_check_arrays(int n, const double *unpx, const double *wpt, const int *scale, const double *Twc)
{
    OV2_REQUIRE(n >= 0, OV2_EINVAL, "negative count (n)");
    OV2_REQUIRE(n <= PNP_MAX_POINTS, OV2_EINVAL, "capacity: more than 2048 points in one problem");
    OV2_REQUIRE(Twc, OV2_EINVAL, "NULL Twc");
    OV2_REQUIRE(n == 0 || (unpx && wpt && scale), OV2_EINVAL, "NULL unpx / wpt / scale");
    for (int c = 0; c < 7; c++) OV2_REQUIRE(std::isfinite(Twc[c]), OV2_EINVAL, "Twc not finite");
    for (size_t i = 0; i < (size_t)n; i++) {
        OV2_REQUIRE(std::isfinite(unpx[2 * i]) && std::isfinite(unpx[2 * i + 1]), OV2_EINVAL, "unpx not finite");
        OV2_REQUIRE(std::isfinite(wpt[3 * i]) && std::isfinite(wpt[3 * i + 1]) && std::isfinite(wpt[3 * i + 2]), OV2_EINVAL, "wpt not finite");
        OV2_REQUIRE(scale[i] >= -60 && scale[i] <= 60, OV2_EINVAL, "|scale| > 60");
    }
    return OV2_OK;
}

static void pnp_fill_args(PnPArgs &a, const ov2_pnp_params *p)
{
    ov2_ba_options o;
    ov2_ba_default_options(&o);
    o.max_iter = p->nmaxiter; o.function_tolerance = 1e-3;
    a.O = ba_opt_from(o);
    a.initial_radius = o.initial_radius;
    a.huber = p->use_robust ? sqrt(p->chi2th) : -1.0;
    a.chi2th = p->chi2th; a.apply_l2 = p->apply_l2_after_robust != 0;
    for (int c = 0; c < 4; c++) a.calib_l[c] = p->K[c];
}

// the pose inputs of problem b, whose points start at pt0, into the host block: [item 16][Twc 56] per item, [unpx 16][wpt 24]
// [sigma 8 = 2^scale] per point.  Both drivers stage them; a PnPItem is a PoseItem whose two flags are 0.
struct PnpIn { size_t o_it, o_tw, o_px, o_wp, o_sg; };
static_assert(sizeof(PnPItem) == sizeof(PoseItem), "one item record for both drivers");
static void pnp_stage_item(uint8_t *hs, const PnpIn &s, int b, const PoseItem &it, const double *Twc, const double *unpx, const double *wpt,
                           const int *scale)
{
    memcpy(hs + s.o_it + sizeof(PoseItem) * b, &it, sizeof(PoseItem));
    memcpy(hs + s.o_tw + 56 * (size_t)b, Twc, 56);
    if (it.n == 0) return;
    memcpy(hs + s.o_px + 16 * (size_t)it.pt0, unpx, 16 * (size_t)it.n);
    memcpy(hs + s.o_wp + 24 * (size_t)it.pt0, wpt, 24 * (size_t)it.n);
    double *sg = (double *)(hs + s.o_sg) + it.pt0;
    for (int i = 0; i < it.n; i++) sg[i] = ldexp(1.0, scale[i]);
}

static void pnp_store_pass(ov2_pnp_pass &d, int ran, int it, int ns, int term, double ic, double fc)
{
    d.ran = ran; d.iterations = it; d.num_successful_steps = ns; d.termination = term; d.initial_cost = ic; d.final_cost = fc;
}

// ---- the chain on a block at capacity (pose_dev.hpp): the lock-step tracker's pose step ---------------------------------------------
int pose_check_params(const ov2_pose_params *params)
{
    OV2_REQUIRE(params, OV2_EINVAL, "NULL params");
    const int rc = pnp_check_params(&params->pnp);  if (rc) return rc;
    P3Plan pl;
    return p3p_plan(&params->p3p, 0, nullptr, nullptr, &pl);
}

int pose_layout(int n_items, int n_max, int n_rows, PoseLayout *L)
{
    const int rc = p3p_plan_capacity(n_items, n_max, n_rows, &L->pl);  if (rc) return rc;
    const size_t B = (size_t)n_items, NP = L->pl.NP;
    L->B = B; L->n_max = n_max; L->n_rows = n_rows;
    StageCursor c(16);
    L->o_it = c.take(sizeof(PoseItem) * B); L->o_px = c.take(16 * NP); L->o_sg = c.take(8 * NP); L->o_p3 = c.take(L->pl.total);
    L->o_cx = c.take(16 * NP); L->o_cw = c.take(24 * NP); L->o_cs = c.take(8 * NP); L->o_ix = c.take(4 * NP);
    L->o_pi = c.take(sizeof(PnPItem) * B); L->o_q0 = c.take(56 * B); L->o_st = c.take(4 * B); L->o_po = c.take(sizeof(PnPOut) * B);
    L->o_pl = c.take(4 * NP); L->o_rm = c.take(NP); L->total = c.off;
    return OV2_OK;
}

int pose_chain_enqueue(hipStream_t s, const ov2_pose_params *params, const PoseLayout &L, uint8_t *ds, const double *Twc_d, PoseOut *out_d,
                       int n_items, bool search)
{
    if (n_items <= 0) return OV2_OK;
    P3Plan pl = L.pl;
    pl.B = (size_t)n_items;                                         // the grids cover the active items; the offsets are the block's
    uint8_t *p3 = ds + L.o_p3;
    if (search) { const int rc = p3p_enqueue(s, &params->p3p, pl, p3);  if (rc) return rc; }
    PoseArgs g;
    g.items = (const PoseItem *)(ds + L.o_it); g.Twc = Twc_d; g.unpx = (const double *)(ds + L.o_px);
    g.wpt = (const double *)(p3 + pl.o_X); g.sigma = (const double *)(ds + L.o_sg);
    g.p3items = search ? (const P3Item *)(p3 + pl.o_it) : nullptr;
    g.p3out = search ? (const P3Out *)(p3 + pl.o_out) : nullptr;
    g.p3ol = search ? (const int *)(p3 + pl.o_ol) : nullptr;
    g.c_unpx = (double *)(ds + L.o_cx); g.c_wpt = (double *)(ds + L.o_cw); g.c_sigma = (double *)(ds + L.o_cs); g.idx = (int *)(ds + L.o_ix);
    g.pnp_items = (PnPItem *)(ds + L.o_pi); g.pose0 = (double *)(ds + L.o_q0); g.stage = (int *)(ds + L.o_st);
    g.pnp_out = (const PnPOut *)(ds + L.o_po); g.pnp_ol = (const int *)(ds + L.o_pl);
    g.out = out_d; g.removed = ds + L.o_rm; g.mono = params->mono != 0;
    hipLaunchKernelGGL(k_pose_gather, dim3(n_items), dim3(64), 0, s, g);
    OV2_HIP_CHECK(hipGetLastError());
    PnPArgs a;
    pnp_fill_args(a, &params->pnp);
    a.items = g.pnp_items; a.pose0 = g.pose0; a.unpx = g.c_unpx; a.wpt = g.c_wpt; a.sigma = g.c_sigma;
    a.out = (PnPOut *)(ds + L.o_po); a.outliers = (int *)(ds + L.o_pl);
    hipLaunchKernelGGL(k_pnp_solve, dim3(n_items), dim3(PNP_THREADS), 0, s, a);
    OV2_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_pose_decide, dim3(n_items), dim3(64), 0, s, g);
    OV2_HIP_CHECK(hipGetLastError());
    return OV2_OK;
}

extern "C" {

int ov2_pose_from_model(const double *model12, double *Twc7)
{
    OV2_REQUIRE(model12 && Twc7, OV2_EINVAL, "NULL argument");
    pose_from_model(model12, Twc7);
    return OV2_OK;
}

int ov2_ceres_pnp_batch(ov2_ctx *ctx, const ov2_pnp_params *params, int n_items, const ov2_pnp_problem *problems, ov2_pnp_result *results)
{
    // the inputs first, the context last: a malformed input is reported without a device
    int rc = pnp_check_params(params);  if (rc) return rc;
    OV2_REQUIRE(n_items >= 0, OV2_EINVAL, "n_items < 0");
    OV2_REQUIRE(n_items == 0 || (problems && results), OV2_EINVAL, "NULL problem / result array");
    OV2_REQUIRE(n_items <= 65535, OV2_EINVAL, "more than 65535 problems in one call");
    size_t NP = 0;
    for (int b = 0; b < n_items; b++) {
        const ov2_pnp_problem &p = problems[b];
        rc = pnp_check_arrays(p.n, p.unpx, p.wpt, p.scale, p.Twc);  if (rc) return rc;
        OV2_REQUIRE(p.n == 0 || results[b].outliers, OV2_EINVAL, "NULL result buffer (outliers)");
        NP += (size_t)p.n;
    }
    OV2_REQUIRE(NP <= 0x7fffffff, OV2_EINVAL, "capacity: more than 2^31 - 1 points in one call");
    OV2_REQUIRE(ctx, OV2_EINVAL, "NULL context");
    if (n_items == 0) return OV2_OK;

    // staging: [items 16 B][pose0 56][unpx 16][wpt 24][sigma 8] up, [out 128][outliers 4] down; every section 16-byte aligned
    const size_t B = (size_t)n_items;
    StageCursor c(16);
    const size_t o_it = c.take(sizeof(PnPItem) * B), o_p0 = c.take(56 * B), o_px = c.take(16 * NP), o_wp = c.take(24 * NP), o_sg = c.take(8 * NP);
    const size_t o_out = c.take(sizeof(PnPOut) * B), o_ol = c.take(4 * NP), total = c.off;
    Stage st;
    rc = st.open(ctx, total, total);  if (rc) return rc;
    uint8_t *hs = st.h, *ds = st.d;
    size_t pt0 = 0;
    for (int b = 0; b < n_items; b++) {
        const ov2_pnp_problem &p = problems[b];
        pnp_stage_item(hs, PnpIn{o_it, o_p0, o_px, o_wp, o_sg}, b, PoseItem{p.n, (int)pt0, 0, 0}, p.Twc, p.unpx, p.wpt, p.scale);
        pt0 += (size_t)p.n;
    }
    rc = st.upload(0, o_out);  if (rc) return rc;
    PnPArgs a;
    pnp_fill_args(a, params);
    a.items = (const PnPItem *)(ds + o_it); a.pose0 = (const double *)(ds + o_p0); a.unpx = (const double *)(ds + o_px);
    a.wpt = (const double *)(ds + o_wp); a.sigma = (const double *)(ds + o_sg); a.out = (PnPOut *)(ds + o_out); a.outliers = (int *)(ds + o_ol);
    hipLaunchKernelGGL(k_pnp_solve, dim3(n_items), dim3(PNP_THREADS), 0, ctx->stream, a);
    OV2_HIP_CHECK(hipGetLastError());
    rc = st.download(o_out, total, o_out);  if (rc) return rc;
    rc = st.sync();  if (rc) return rc;
    pt0 = 0;
    for (int b = 0; b < n_items; b++) {
        const ov2_pnp_problem &p = problems[b];
        ov2_pnp_result &r = results[b];
        PnPOut o;
        memcpy(&o, hs + o_out + sizeof(PnPOut) * b, sizeof(PnPOut));
        r.success = o.success; r.n_outliers = o.n_out;
        memcpy(r.Twc, o.pose, 56);
        if (o.n_out > 0) memcpy(r.outliers, hs + o_ol + 4 * pt0, 4 * (size_t)o.n_out);
        for (int q = 0; q < 2; q++) pnp_store_pass(r.pass[q], o.ran[q], o.iterations[q], o.n_success[q], o.termination[q], o.initial_cost[q], o.final_cost[q]);
        pt0 += (size_t)p.n;
    }
    return OV2_OK;
}

int ov2_ceres_pnp(ov2_ctx *ctx, const ov2_pnp_params *params, const ov2_pnp_problem *problem, ov2_pnp_result *result)
{
    OV2_REQUIRE(problem && result, OV2_EINVAL, "NULL problem / result");
    return ov2_ceres_pnp_batch(ctx, params, 1, problem, result);
}

int ov2_compute_pose_batch(ov2_ctx *ctx, const ov2_pose_params *params, int n_items, const ov2_pose_problem *problems, ov2_pose_result *results)
{
    OV2_REQUIRE(params, OV2_EINVAL, "NULL params");
    int rc = pnp_check_params(&params->pnp);  if (rc) return rc;
    OV2_REQUIRE(n_items >= 0, OV2_EINVAL, "n_items < 0");
    OV2_REQUIRE(n_items == 0 || (problems && results), OV2_EINVAL, "NULL problem / result array");
    OV2_REQUIRE(n_items <= 65535, OV2_EINVAL, "more than 65535 problems in one call");
    size_t NP = 0;
    bool any_p3p = false;
    std::vector<ov2_p3p_problem> search((size_t)n_items);           // the items that search; the others as empty problems
    for (int b = 0; b < n_items; b++) {
        const ov2_pose_problem &p = problems[b];
        rc = pnp_check_arrays(p.n, p.unpx, p.wpt, p.scale, p.Twc);  if (rc) return rc;
        OV2_REQUIRE(p.n == 0 || results[b].removed, OV2_EINVAL, "NULL result buffer (removed)");
        ov2_p3p_problem &s = search[(size_t)b];
        s = ov2_p3p_problem{0, nullptr, nullptr, 0, nullptr};
        if (p.do_p3p) OV2_REQUIRE(p.n_rows >= 0, OV2_EINVAL, "negative count (n / n_rows)");
        if (p.do_p3p && p.n >= 4) {
            s.n = p.n; s.bv = p.bv; s.X = p.wpt; s.n_rows = p.n_rows; s.samples = p.samples;
            any_p3p = true;
        }
        NP += (size_t)p.n;
    }
    OV2_REQUIRE(NP <= 0x7fffffff, OV2_EINVAL, "capacity: more than 2^31 - 1 points in one call");
    P3Plan pl;
    rc = p3p_plan(&params->p3p, n_items, search.data(), nullptr, &pl);  if (rc) return rc;
    OV2_REQUIRE(ctx, OV2_EINVAL, "NULL context");
    if (n_items == 0) return OV2_OK;

    // device: [pose inputs: items 16 B, Twc 56, unpx 16, wpt 24, sigma 8][the search's block, its inputs first] -- ONE upload up to
    // here -- [the rest of the search's block][compacted unpx, wpt, sigma, idx 4][PnP items 16, pose0 56, stage 4, PnP out 128,
    // PnP outliers 4][out 168, removed 1] -- ONE download of the last two
    const size_t B = (size_t)n_items;
    StageCursor c(16);
    const size_t o_it = c.take(sizeof(PoseItem) * B), o_tw = c.take(56 * B), o_px = c.take(16 * NP), o_wp = c.take(24 * NP), o_sg = c.take(8 * NP);
    const size_t o_p3 = c.take(any_p3p ? pl.total : 0), up_end = o_p3 + (any_p3p ? pl.o_out : 0);
    const size_t o_cx = c.take(16 * NP), o_cw = c.take(24 * NP), o_cs = c.take(8 * NP), o_ix = c.take(4 * NP);
    const size_t o_pi = c.take(sizeof(PnPItem) * B), o_q0 = c.take(56 * B), o_st = c.take(4 * B), o_po = c.take(sizeof(PnPOut) * B);
    const size_t o_pl = c.take(4 * NP), o_out = c.take(sizeof(PoseOut) * B), o_rm = c.take(NP), total = c.off;
    Stage st;
    rc = st.open(ctx, total, up_end + (total - o_out));  if (rc) return rc;
    uint8_t *hs = st.h, *ds = st.d, *hd = hs + up_end;   // hd: where [o_out, total) comes down
    size_t pt0 = 0;
    for (int b = 0; b < n_items; b++) {
        const ov2_pose_problem &p = problems[b];
        pnp_stage_item(hs, PnpIn{o_it, o_tw, o_px, o_wp, o_sg}, b, PoseItem{p.n, (int)pt0, p.do_p3p != 0, p.p3p_req != 0}, p.Twc, p.unpx, p.wpt,
                       p.scale);
        pt0 += (size_t)p.n;
    }
    if (any_p3p) p3p_stage(pl, search.data(), hs + o_p3);
    rc = st.upload(0, up_end);  if (rc) return rc;
    if (any_p3p) { rc = p3p_enqueue(ctx->stream, &params->p3p, pl, ds + o_p3);  if (rc) return rc; }
    PoseArgs g;
    g.items = (const PoseItem *)(ds + o_it); g.Twc = (const double *)(ds + o_tw); g.unpx = (const double *)(ds + o_px);
    g.wpt = (const double *)(ds + o_wp); g.sigma = (const double *)(ds + o_sg);
    g.p3items = any_p3p ? (const P3Item *)(ds + o_p3 + pl.o_it) : nullptr;
    g.p3out = any_p3p ? (const P3Out *)(ds + o_p3 + pl.o_out) : nullptr;
    g.p3ol = any_p3p ? (const int *)(ds + o_p3 + pl.o_ol) : nullptr;
    g.c_unpx = (double *)(ds + o_cx); g.c_wpt = (double *)(ds + o_cw); g.c_sigma = (double *)(ds + o_cs); g.idx = (int *)(ds + o_ix);
    g.pnp_items = (PnPItem *)(ds + o_pi); g.pose0 = (double *)(ds + o_q0); g.stage = (int *)(ds + o_st);
    g.pnp_out = (const PnPOut *)(ds + o_po); g.pnp_ol = (const int *)(ds + o_pl);
    g.out = (PoseOut *)(ds + o_out); g.removed = ds + o_rm; g.mono = params->mono != 0;
    hipLaunchKernelGGL(k_pose_gather, dim3(n_items), dim3(64), 0, ctx->stream, g);
    OV2_HIP_CHECK(hipGetLastError());
    PnPArgs a;
    pnp_fill_args(a, &params->pnp);
    a.items = g.pnp_items; a.pose0 = g.pose0; a.unpx = g.c_unpx; a.wpt = g.c_wpt; a.sigma = g.c_sigma;
    a.out = (PnPOut *)(ds + o_po); a.outliers = (int *)(ds + o_pl);
    hipLaunchKernelGGL(k_pnp_solve, dim3(n_items), dim3(PNP_THREADS), 0, ctx->stream, a);
    OV2_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_pose_decide, dim3(n_items), dim3(64), 0, ctx->stream, g);
    OV2_HIP_CHECK(hipGetLastError());
    rc = st.download(o_out, total, up_end);  if (rc) return rc;
    rc = st.sync();  if (rc) return rc;
    pt0 = 0;
    for (int b = 0; b < n_items; b++) {
        const ov2_pose_problem &p = problems[b];
        ov2_pose_result &r = results[b];
        PoseOut o;
        memcpy(&o, hd + sizeof(PoseOut) * b, sizeof(PoseOut));
        memcpy(r.Twc, o.Twc, 56);
        r.action = o.action; r.p3p_req_out = o.p3p_req_out; r.n_removed_p3p = o.n_removed_p3p; r.n_outliers_pnp = o.n_outliers_pnp;
        r.ran_p3p = o.ran_p3p; r.p3p_status = o.p3p_status; r.p3p_best_row = o.p3p_best_row; r.p3p_iterations = o.p3p_iterations;
        r.p3p_rows_consumed = o.p3p_rows_consumed; r.p3p_score = o.p3p_score;
        if (p.n) memcpy(r.removed, hd + (o_rm - o_out) + pt0, (size_t)p.n);
        for (int q = 0; q < 2; q++) pnp_store_pass(r.pass[q], o.ran[q], o.iterations[q], o.n_success[q], o.termination[q], o.initial_cost[q], o.final_cost[q]);
        pt0 += (size_t)p.n;
    }
    return OV2_OK;
}

int ov2_compute_pose(ov2_ctx *ctx, const ov2_pose_params *params, const ov2_pose_problem *problem, ov2_pose_result *result)
{
    OV2_REQUIRE(problem && result, OV2_EINVAL, "NULL problem / result");
    return ov2_compute_pose_batch(ctx, params, 1, problem, result);
}

}  // extern "C"
