// ba_local.hpp -- Optimizer::localBA's two-pass protocol on the device: one problem (local_ba_one) and a lock-step batch of
// problems that share every launch (local_ba_batch).  A part of ba.hip (same translation unit): included there after ba_run.
#pragma once
#include <string>
// ================================================================================== lock-step batch of local-BA problems
// BASELINE configs[4]: eleven sequences advance in lock step on one GPU (ov2_btracker_*), their keyframes arrive together -- and
// eleven estimator threads with a stream each then push ~100 launches per solve through the command processor, where they queue
// behind each other and behind the front end's (round 5: 5.8 ms of wall clock per 0.9 ms solve, the SLAM thread 1.8x slower).
// Here the problems of one step share every launch: blockIdx.z = problem, the kernels read their BADev from an array in device
// memory instead of the kernel arguments, a problem that has converged (or takes no second pass) leaves through the kernels'
// `if (ctl->done) return`.  The one-work-group kernels (factorisation, bookkeeping) so run on as many CUs as there are problems.
// The arithmetic of a problem is that of ov2_local_ba (same device functions); grids are the largest any problem of the batch
// needs, the per-work-group partial sums are added in a different grouping when a problem runs on a larger grid than alone.
// The host side is local_ba_batch's steps: one that fails hands its code back and becomes the status of the problems it concerns.

// results of the batch into ONE block (ba_out_layout per problem): one download instead of three to five small ones per problem
__global__ __launch_bounds__(256) void k_ba_gather_B(const BADev *__restrict__ arr)
{
    const BADev &D = arr[blockIdx.z];
    const unsigned i0 = blockIdx.x * blockDim.x + threadIdx.x;          // (the grid is 64 work-groups at most: ba_batch_fetch)
    const long long stride = (long long)gridDim.x * blockDim.x;
    const BAOutLayout L = ba_out_layout(D.n_kf, D.n_lm, D.n_res, D.out_flags);
    uint8_t *o = D.out_b;
    for (long long e = i0; e < 7LL * D.n_kf; e += stride) ((double *)(o + L.poses))[e] = D.x_pose[e];
    for (long long e = i0; e < D.n_lm; e += stride) ((double *)(o + L.invdepth))[e] = D.x_lam[e];
    for (long long e = i0; e < D.n_res; e += stride) (o + L.bad_obs)[e] = D.bad_obs[e];
    if (D.out_flags & 1) for (long long e = i0; e < D.n_res; e += stride) ((double *)(o + L.chi2))[e] = D.chi2[e];
    if (D.out_flags & 2) for (long long e = i0; e < D.n_res; e += stride) (o + L.dpos)[e] = D.dpos[e];
}

struct BAMember {                                       // a problem that shares the batch's launches
    int i, out_flags;                                   // which problem of the call; optional parts of its results: 1: chi2, 2: depth flags
    ov2_ba_dev *dev = nullptr; size_t out_off = 0;      // on the device; its slot of the result block
    double huber = -1.0; uint8_t skip = 0;              // Huber's delta of the pass to come; sits the second pass out
};

struct BABatch {
    std::vector<BAMember> m;
    BADev *h_arr = nullptr, *d_arr = nullptr;           // the problems' device views: pinned staging / device copy
    BACtl *h_ctl = nullptr, *d_ctl = nullptr;           // control blocks, consecutive (one download per pass)
    int *h_cnt = nullptr, *d_cnt = nullptr;             // 16 counters per problem (k_ba_mark_outliers)
    volatile int *h_flag = nullptr;                     // the look-ahead words of k_ba_decide
    size_t out_base = 0, out_total = 0;                 // the result block (k_ba_gather_B) inside the two blocks
    ~BABatch() { for (BAMember &q : m) ba_destroy(q.dev); }
};

// the launch geometry of a pass of the batch, and the members' views for it into the pinned array
static int ba_batch_views(BABatch &B, const ov2_ba_options *o, bool second, BAGeom &G)
{
    const int N = (int)B.m.size();
    // a single problem spreads over the whole chip for latency (16 landmarks per lineariser work-group, 1024 Schur work-groups); a batch
    // fills it anyway: ~768 lineariser and ~2048 Schur work-groups over ALL problems -- fewer flushes of the LDS aggregates and fewer
    // atomic adds into G per problem (eleven windows: 2.31 -> 2.07 ms of device time; tools/r5_ba_batch_grid.sh swept 512 .. 4096 / 1024 .. 16384)
    const int lin_total = 768, schur_total = 2048;
    const int lin_cap = std::max(16, std::min(256, (lin_total + N - 1) / N));
    const int schur_wgs = std::max(64, std::min(1024, (schur_total + N - 1) / N));
    // grids and LDS bytes: the largest any problem needs; the Schur split is each problem's own (into its view)
    std::vector<BAGeom> each((size_t)N);
    for (int i = 0; i < N; i++) each[(size_t)i] = ba_geom(B.m[(size_t)i].dev->D, lin_cap, schur_wgs);
    G = each[0];
    for (int i = 1; i < N; i++) ba_geom_max(G, each[(size_t)i]);
    OV2_REQUIRE(G.lin_lds <= BA_LIN_LDS_MAX && G.chol_lds <= BA_CHOL_LDS_MAX, OV2_EUNSUPPORTED, "a problem of the batch is too large for the LDS-resident path");
    for (int i = 0; i < N; i++) {
        const BAMember &q = B.m[(size_t)i];
        BADev D = q.dev->D;
        const BAGeom &g = each[(size_t)i];
        ba_view_for_solve(D, o, q.huber, G);
        D.g_ntiles = g.ntiles; D.g_nupper = g.n_upper; D.g_lmps = g.lm_per_split; D.g_ksplit = g.ksplit;
        D.skip2 = second && q.skip ? 1 : 0;
        D.flag_h = (int *)(B.h_flag + i);
        D.ctl = B.d_ctl + i; D.lba_cnt = B.d_cnt + 16 * i;
        B.h_arr[i] = D;
        B.h_flag[i] = -1;
    }
    return OV2_OK;
}

// one LM solve of every problem of the batch (ba_run's loop on batched launches).  second: the pass after the first outlier test --
// it continues from the state on the device, landmarks that lost all their blocks leave the program first, members with `skip` sit it out
static int ba_run_batch(ov2_ctx *ctx, BABatch &B, const ov2_ba_options *o, bool second, float *ms_out)
{
    int rc = ba_check_options(o);
    if (rc == OV2_OK) rc = ba_raise_lds_limits();
    if (rc == OV2_OK) rc = ba_events(ctx);
    if (rc != OV2_OK) return rc;
    const int N = (int)B.m.size();
    hipStream_t s = ctx->stream;
    const BAOpt O = ba_opt_from(*o);
    BAGeom G;
    rc = ba_batch_views(B, o, second, G);
    if (rc != OV2_OK) return rc;
    OV2_HIP_CHECK(hipMemcpyAsync(B.d_arr, B.h_arr, sizeof(BADev) * (size_t)N, hipMemcpyHostToDevice, s));
    OV2_HIP_CHECK(hipEventRecord(ctx->ba_ev[0], s));
    BACtl c0;
    ba_ctl_init(c0, o->initial_radius, nullptr);
    const BADev *A = B.d_arr;
    const unsigned Z = (unsigned)N;
    if (second) {
        // (skip2 reaches the device with the upload of the views above: k_ba_lm_live_B runs after it, as part of the reset)
        int ll = 1;
        for (const BAMember &q : B.m) ll = std::max(ll, std::min(512, (q.dev->D.n_lm + 3) / 4));
        hipLaunchKernelGGL(k_ba_lm_live_B, dim3(ll, 1, Z), dim3(256), 0, s, A);
    }
    hipLaunchKernelGGL(k_ba_reset_B, dim3(G.reset_blocks_B, 1, Z), dim3(256), 0, s, A, c0, second ? 1 : 0);
    hipLaunchKernelGGL(k_ba_init_B, dim3(G.init_blocks, 1, Z), dim3(256), 0, s, A);
    auto linearize = [&]() { hipLaunchKernelGGL(k_ba_linearize_B, dim3(G.lin_blocks, 1, Z), dim3(256), G.lin_lds, s, A); };
    auto first_half = [&](int it) {
        hipLaunchKernelGGL(k_ba_iter_begin_B, dim3(1, 1, Z), dim3(1024), 0, s, A, O, it);
        hipLaunchKernelGGL(k_ba_schur_gemm_B, dim3(G.n_upper, G.ksplit, Z), dim3(256), 0, s, A);
        hipLaunchKernelGGL(k_ba_assemble_B, dim3((G.nf + 255) / 256, G.nf, Z), dim3(256), 0, s, A);
        hipLaunchKernelGGL(k_ba_cholesky_B, dim3(1, 1, Z), dim3(512), G.chol_lds, s, A);
    };
    auto second_half = [&](int it) {
        hipLaunchKernelGGL(k_ba_backsub_B, dim3(G.bs_blocks, 1, Z), dim3(256), G.bs_lds, s, A);
        hipLaunchKernelGGL(k_ba_candidate_B, dim3(1, 1, Z), dim3(1024), 0, s, A, O);
        hipLaunchKernelGGL(k_ba_cost_B, dim3(G.cost_blocks, 1, Z), dim3(256), 0, s, A);
        hipLaunchKernelGGL(k_ba_decide_B, dim3(1, 1, Z), dim3(1024), 0, s, A, O, it);
        linearize();
    };
    linearize();
    rc = ba_lm_loop(s, o, O, B.h_flag, N, first_half, second_half,
                    [&](const BAOpt &Ob) { hipLaunchKernelGGL(k_ba_iter_begin_B, dim3(1, 1, Z), dim3(1024), 0, s, A, Ob, -1); });
    if (rc != OV2_OK) return rc;
    OV2_HIP_CHECK(hipEventRecord(ctx->ba_ev[1], s));
    OV2_HIP_CHECK(hipMemcpyAsync(B.h_ctl, B.d_ctl, sizeof(BACtl) * (size_t)N, hipMemcpyDeviceToHost, s));
    OV2_HIP_CHECK(hipStreamSynchronize(s));
    OV2_HIP_CHECK(hipEventElapsedTime(ms_out, ctx->ba_ev[0], ctx->ba_ev[1]));
    return OV2_OK;
}

// ---------------------------------------------------------------------------------- the two-pass localBA protocol, per problem
// What both drivers do between their launches; the launches differ (one problem's kernels / the batch's), this bookkeeping does not.
static void local_ba_clear_result(ov2_local_ba_result &r)
{
    r.l2_done = 0; r.pass2_error = OV2_OK; r.n_bad_pass1 = 0; r.n_bad_total = 0; r.status = OV2_OK;
    for (int q = 0; q < 2; q++) { r.iterations[q] = 0; r.num_successful_steps[q] = 0; r.termination[q] = OV2_TERM_NO_CONVERGENCE; r.initial_cost[q] = r.final_cost[q] = 0; r.solve_ms[q] = 0; }
}

// the summary of a finished pass (q = 0, 1) into its slot
static void local_ba_store_pass(ov2_local_ba_result &r, int q, const ov2_ba_result &b)
{
    r.iterations[q] = b.iterations; r.num_successful_steps[q] = b.num_successful_steps; r.termination[q] = b.termination;
    r.initial_cost[q] = b.initial_cost; r.final_cost[q] = b.final_cost; r.solve_ms[q] = b.solve_ms;
}
static ov2_ba_result ba_pass_summary(const BACtl &c, float ms) { ov2_ba_result b{}; ba_fill_result(&b, c, ms); return b; }

// Huber's delta of the first pass (<= 0: trivial loss)
static double local_ba_huber(const ov2_local_ba_options &o) { return o.use_robust_cost ? sqrt(o.robust_mono_th) : -1.0; }

// After the first outlier test (src/optimizer.cpp:603-608); cnt: outliers, left-camera blocks that remain, right-camera blocks that
// remain.  Is there a second pass, and with which loss?  stopLocalBA() is evaluated HERE, after the first solve: a keyframe that
// arrived while pass 1 ran skips pass 2.  The loss is reset to L2 only when both residual lists are still non-empty (mono runs keep Huber!).
static bool local_ba_first_test(const ov2_local_ba_options &o, const int *cnt, ov2_local_ba_result &r, double *huber2)
{
    r.n_bad_pass1 = r.n_bad_total = cnt[0];
    const bool stop = o.stop_requested || (o.stop_flag && *o.stop_flag);
    *huber2 = (cnt[1] && cnt[2]) ? -1.0 : local_ba_huber(o);
    return o.apply_l2_after_robust && o.use_robust_cost && !stop && cnt[0] > 0;
}

// A second pass that was started.  It could not run (rc): the device still holds an accepted state (pass 1's, or a later accepted
// LM step) and the verdicts of the first test -- the caller hands those back instead of dropping a valid solve, and runs no second test.
static void local_ba_pass2(ov2_local_ba_result &r, int rc, const ov2_ba_result &b)
{
    if (rc != OV2_OK) { r.pass2_error = rc; return; }
    r.l2_done = 1;
    local_ba_store_pass(r, 1, b);
}

// the second outlier test (:637-735) counted the blocks that were still in the problem
static void local_ba_second_test(ov2_local_ba_result &r, int n_bad2)
{
    if (r.l2_done) r.n_bad_total = r.n_bad_pass1 + n_bad2;
}

// the outlier test of one problem, and its counters (16 bytes) on their way to the host
static int ba_mark_outliers(hipStream_t s, const BADev &D, double th, int deactivate, int *cnt_h)
{
    const int mk_blocks = std::max(1, std::min(1024, (D.n_act + 255) / 256));
    hipLaunchKernelGGL(k_ba_mark_outliers, dim3(mk_blocks), dim3(256), 0, s, D, th, deactivate, (uint8_t *)nullptr);
    OV2_HIP_CHECK(hipGetLastError());
    OV2_HIP_CHECK(hipMemcpyAsync(cnt_h, D.lba_cnt, 16, hipMemcpyDeviceToHost, s));
    return OV2_OK;
}
// ... of every member of a batch
static int ba_mark_outliers_B(hipStream_t s, const BABatch &B, double th, int deactivate)
{
    const size_t N = B.m.size();
    int mk_blocks = 1;
    for (const BAMember &q : B.m) mk_blocks = std::max(mk_blocks, std::min(1024, (q.dev->D.n_act + 255) / 256));
    hipLaunchKernelGGL(k_ba_mark_outliers_B, dim3(mk_blocks, 1, (unsigned)N), dim3(256), 0, s, (const BADev *)B.d_arr, th, deactivate, (uint8_t *)nullptr);
    OV2_HIP_CHECK(hipGetLastError());
    OV2_HIP_CHECK(hipMemcpyAsync(B.h_cnt, B.d_cnt, 64 * N, hipMemcpyDeviceToHost, s));
    return OV2_OK;
}

// Optimizer::localBA's solve stage (src/optimizer.cpp:436-735) with the problem RESIDENT between the two passes: one
// counting sort + one upload, the outlier tests and the removal of residual blocks on the device, one download.
static int local_ba_one(ov2_ctx *ctx, const ov2_ba_problem *p, const ov2_local_ba_options *o, ov2_local_ba_result *r)
{
    local_ba_clear_result(*r);
    OV2_REQUIRE(o->robust_mono_th > 0, OV2_EINVAL, "robust_mono_th must be positive");
    ov2_ba_dev *dev = nullptr;
    const BALap lap{"local_ba", ctx->debug != 0};
    int rc = ba_create(ctx, p, &dev, /*transient*/ true);       // the pool lives in the context's scratch through both passes
    if (rc != OV2_OK) return rc;
    lap("sort + upload (ba_create)");
    struct Guard { ov2_ba_dev *d; ~Guard() { ba_destroy(d); } } guard{dev};
    if (dev->D.n_po > 0) { ov2_set_error("ov2_local_ba: problems with OV2_RES_PNP blocks go through ov2_ba_solve"); return OV2_EUNSUPPORTED; }
    BADev &D = dev->D;
    hipStream_t s = ctx->stream;
    // pass 1 (:436-485)
    ov2_ba_options o1 = o->pass1, o2 = o->pass2;
    o1.huber_delta = local_ba_huber(*o);
    ov2_ba_result br{};
    rc = ba_run(ctx, dev, &o1, &br, nullptr, nullptr);
    if (rc != OV2_OK) return rc;
    local_ba_store_pass(*r, 0, br);
    lap("pass 1");
    // outlier test on the values cached by the last Evaluate of pass 1 (:492-594)
    rc = ctx->reserve_host(64);
    if (rc != OV2_OK) return rc;
    int *cnt_h = (int *)ctx->h_scratch;
    rc = ba_mark_outliers(s, D, o->robust_mono_th, o->apply_l2_after_robust ? 1 : 0, cnt_h);
    if (rc != OV2_OK) return rc;
    if (r->bad_after_pass1 && dev->n_res > 0) OV2_HIP_CHECK(hipMemcpyAsync(r->bad_after_pass1, D.bad_obs, (size_t)dev->n_res, hipMemcpyDeviceToHost, s));
    OV2_HIP_CHECK(hipStreamSynchronize(s));
    lap("outlier test 1");
    if (local_ba_first_test(*o, cnt_h, *r, &o2.huber_delta)) {
        hipLaunchKernelGGL(k_ba_lm_live, dim3(std::max(1, std::min(512, (D.n_lm + 3) / 4))), dim3(256), 0, s, D);
        OV2_HIP_CHECK(hipMemsetAsync(D.lba_cnt, 0, 16, s));
        rc = ba_run(ctx, dev, &o2, &br, nullptr, nullptr, /*keep_state*/ true);
        local_ba_pass2(*r, rc, br);
        if (rc == OV2_OK) {
            lap("pass 2");
            // second outlier test on the residual blocks that are still in the problem (:637-735)
            rc = ba_mark_outliers(s, D, o->robust_mono_th, 0, cnt_h);
            if (rc != OV2_OK) return rc;
        }
    }
    rc = ba_download(s, dev, r->poses_out, r->invdepth_out, r->bad_obs, r->chi2_last_eval, r->depthpos_last_eval);
    if (rc != OV2_OK) return rc;
    OV2_HIP_CHECK(hipStreamSynchronize(s));
    local_ba_second_test(*r, cnt_h[0]);
    lap("outlier test 2 + download");
    return OV2_OK;
}

// ---------------------------------------------------------------------------------- the batch's steps
static bool same_solver_options(const ov2_ba_options &a, const ov2_ba_options &b)
{
    return a.max_iter == b.max_iter && a.function_tolerance == b.function_tolerance && a.gradient_tolerance == b.gradient_tolerance &&
           a.parameter_tolerance == b.parameter_tolerance && a.initial_radius == b.initial_radius && a.max_radius == b.max_radius &&
           a.min_radius == b.min_radius && a.min_lm_diagonal == b.min_lm_diagonal && a.max_lm_diagonal == b.max_lm_diagonal &&
           a.min_relative_decrease == b.min_relative_decrease && a.jacobi_scaling == b.jacobi_scaling &&
           a.max_consecutive_invalid_steps == b.max_consecutive_invalid_steps && a.max_solver_time_s == b.max_solver_time_s;
}

// what concerns the batch as a whole
static int local_ba_check_batch(ov2_ctx *ctx, int n, const ov2_local_ba_options *o)
{
    for (int i = 0; i < n; i++) {
        OV2_REQUIRE(o[i].robust_mono_th > 0, OV2_EINVAL, "robust_mono_th must be positive");
        OV2_REQUIRE(o[i].robust_mono_th == o[0].robust_mono_th && o[i].use_robust_cost == o[0].use_robust_cost && o[i].apply_l2_after_robust == o[0].apply_l2_after_robust &&
                    same_solver_options(o[i].pass1, o[0].pass1) && same_solver_options(o[i].pass2, o[0].pass2), OV2_EINVAL,
                    "ov2_local_ba_batch: the problems of a batch share the protocol and solver options (only the stop request is per problem)");
    }
    OV2_HIP_CHECK(hipSetDevice(ctx->device));
    return OV2_OK;
}

// which problems can share launches: inverse-depth problems of the LDS-resident path with landmarks and optimised keyframes; the
// others are marked in `alone`
static std::vector<BAMember> local_ba_classify(const ov2_ctx *ctx, int n, const ov2_ba_problem *p, const ov2_local_ba_result *r, std::vector<uint8_t> &alone)
{
    std::vector<BAMember> m;
    alone.assign((size_t)n, 0);
    for (int i = 0; i < n; i++) {
        int n_opt = 0;
        if (p[i].n_kf > 0 && p[i].kf_const) for (int k = 0; k < p[i].n_kf; k++) n_opt += !p[i].kf_const[k];
        const bool ok = !ctx->ba_deterministic && !ctx->ba_force_large && p[i].n_lm > 0 && p[i].n_res > 0 && n_opt > 0 && ba_small_path(n_opt);
        if (ok) m.push_back(BAMember{i, (r[i].chi2_last_eval ? 1 : 0) | (r[i].depthpos_last_eval ? 2 : 0)});
        else alone[(size_t)i] = 1;
    }
    return m;
}

// the host side of every member (validation, the landmark sort, the staging mirror; ~0.4 ms for a 69 k-block window) on a thread of
// its own (sixteen persistent threads of the context) -- on one thread it was more than the batch's device time.  Each thread enqueues
// its problem's upload on the context's stream itself (the order of the uploads does not matter).  rcs / errs: ba_create's answers
static void ba_batch_create(ov2_ctx *ctx, BABatch &B, const ov2_ba_problem *p, BASlice &sl, std::vector<int> &rcs, std::vector<std::string> &errs)
{
    const size_t N = B.m.size();
    rcs.assign(N, OV2_OK);
    errs.assign(N, std::string());
    BAHostPool *hp = N > 1 ? ba_host_pool_of(ctx) : nullptr;
    const std::function<void(int)> work = [&](int k) {
        (void)hipSetDevice(ctx->device);
        BAMember &q = B.m[(size_t)k];
        rcs[(size_t)k] = ba_create(ctx, &p[q.i], &q.dev, true, &sl);
        if (rcs[(size_t)k] != OV2_OK && rcs[(size_t)k] != BA_SLICE_FULL) errs[(size_t)k] = ov2_last_error();          // (the message is per thread)
    };
    if (hp) hp->run((int)N, work);
    else for (size_t k = 0; k < N; k++) work((int)k);
}

// The batch's two blocks and its members on the device: header (ba_batch_header) | result block | the problems' slices, in the
// context's pinned and device scratch.  A block that turns out too small grows and everything starts over (the first batches of a run
// only); a member that ba_create rejects gets its code as its status and leaves, the others start over without it.  Members that turn
// out large or to carry pose-only blocks go to `alone`.  A failure concerns every member that is left.
static int ba_batch_build(ov2_ctx *ctx, BABatch &B, const ov2_ba_problem *p, ov2_local_ba_result *r, std::vector<uint8_t> &alone)
{
    hipStream_t s = ctx->stream;
    size_t host_need = 0, dev_need = 0;
    while (!B.m.empty()) {
        const BABatchHeader H = ba_batch_header((int)B.m.size(), sizeof(BACtl), sizeof(BADev));
        B.out_base = H.out_base; B.out_total = 0;
        for (BAMember &q : B.m) { q.out_off = B.out_total; B.out_total += ba_out_layout(p[q.i].n_kf, p[q.i].n_lm, p[q.i].n_res, q.out_flags).total; }
        const size_t header = H.out_base + ba_up256(B.out_total);
        int rc = ctx->reserve_host(std::max(std::max(header, host_need), ctx->h_scratch_bytes));
        if (rc == OV2_OK) rc = ctx->reserve_device(std::max(std::max(header, dev_need), ctx->d_scratch_bytes));
        if (rc != OV2_OK) return rc;
        uint8_t *hb = (uint8_t *)ctx->h_scratch, *db = (uint8_t *)ctx->d_scratch;
        B.h_flag = (volatile int *)(hb + H.flag); B.h_cnt = (int *)(hb + H.cnt); B.h_ctl = (BACtl *)(hb + H.ctl); B.h_arr = (BADev *)(hb + H.arr);
        B.d_cnt = (int *)(db + H.cnt); B.d_ctl = (BACtl *)(db + H.ctl); B.d_arr = (BADev *)(db + H.arr);
        BASlice sl;
        sl.dev_base = db; sl.dev_cap = ctx->d_scratch_bytes; sl.dev_used = header; sl.host_base = hb; sl.host_cap = ctx->h_scratch_bytes; sl.host_used = header;
        std::vector<int> rcs;
        std::vector<std::string> errs;
        ba_batch_create(ctx, B, p, sl, rcs, errs);
        if (std::all_of(rcs.begin(), rcs.end(), [](int c) { return c == OV2_OK; })) {
            for (BAMember &q : B.m) { q.dev->D.out_b = db + B.out_base + q.out_off; q.dev->D.out_flags = q.out_flags; }
            break;
        }
        OV2_HIP_CHECK(hipStreamSynchronize(s));
        for (BAMember &q : B.m) { ba_destroy(q.dev); q.dev = nullptr; }
        for (size_t k = B.m.size(); k-- > 0;) {
            if (rcs[k] == OV2_OK || rcs[k] == BA_SLICE_FULL) continue;
            r[B.m[k].i].status = rcs[k];
            ov2_set_error("ov2_local_ba_batch: problem %d: %s", B.m[k].i, errs[k].c_str());
            B.m.erase(B.m.begin() + (long)k);
        }
        // grow-only blocks: twice what this batch would have taken
        if (std::find(rcs.begin(), rcs.end(), BA_SLICE_FULL) != rcs.end()) { host_need = 2 * sl.host_used; dev_need = 2 * sl.dev_used; }
    }
    for (size_t k = 0; k < B.m.size();) {
        const BADev &D = B.m[k].dev->D;
        if (D.n_po == 0 && !D.big) { k++; continue; }
        alone[(size_t)B.m[k].i] = 1;
        OV2_HIP_CHECK(hipStreamSynchronize(s));
        ba_destroy(B.m[k].dev);
        B.m.erase(B.m.begin() + (long)k);
    }
    return OV2_OK;
}

// both passes and both outlier tests of the members, on shared launches (only the stop request is per problem: the other options
// are the batch's).  A second pass that fails is no failure of the step: local_ba_pass2
static int local_ba_shared(ov2_ctx *ctx, BABatch &B, const ov2_local_ba_options *o, ov2_local_ba_result *r, const BALap &lap)
{
    hipStream_t s = ctx->stream;
    const size_t N = B.m.size();
    const ov2_local_ba_options &o0 = o[0];
    for (BAMember &q : B.m) { q.huber = local_ba_huber(o0); q.skip = 0; }
    OV2_HIP_CHECK(hipMemsetAsync(B.d_cnt, 0, 64 * N, s));
    float ms = 0;
    int rc = ba_run_batch(ctx, B, &o0.pass1, false, &ms);
    if (rc != OV2_OK) return rc;
    lap("pass 1");
    for (size_t k = 0; k < N; k++) local_ba_store_pass(r[B.m[k].i], 0, ba_pass_summary(B.h_ctl[k], ms));
    rc = ba_mark_outliers_B(s, B, o0.robust_mono_th, o0.apply_l2_after_robust ? 1 : 0);
    if (rc != OV2_OK) return rc;
    for (const BAMember &q : B.m)
        if (r[q.i].bad_after_pass1 && q.dev->n_res > 0) OV2_HIP_CHECK(hipMemcpyAsync(r[q.i].bad_after_pass1, q.dev->D.bad_obs, (size_t)q.dev->n_res, hipMemcpyDeviceToHost, s));
    OV2_HIP_CHECK(hipStreamSynchronize(s));
    lap("outlier test 1");
    int n_pass2 = 0;
    for (size_t k = 0; k < N; k++) {
        BAMember &q = B.m[k];
        const bool go = local_ba_first_test(o[q.i], B.h_cnt + 16 * k, r[q.i], &q.huber);
        q.skip = go ? 0 : 1;
        n_pass2 += go;
    }
    if (n_pass2 == 0) return OV2_OK;
    OV2_HIP_CHECK(hipMemsetAsync(B.d_cnt, 0, 64 * N, s));
    rc = ba_run_batch(ctx, B, &o0.pass2, true, &ms);
    lap("pass 2");
    for (size_t k = 0; k < N; k++) if (!B.m[k].skip) local_ba_pass2(r[B.m[k].i], rc, ba_pass_summary(B.h_ctl[k], ms));
    return rc == OV2_OK ? ba_mark_outliers_B(s, B, o0.robust_mono_th, 0) : OV2_OK;
}

// the members' results: one gather, one download, then each part to where its problem wants it
static int ba_batch_fetch(ov2_ctx *ctx, const BABatch &B, ov2_local_ba_result *r)
{
    hipStream_t s = ctx->stream;
    int gb = 1;
    for (const BAMember &q : B.m) gb = std::max(gb, std::min(64, (std::max(q.dev->D.n_res, q.dev->D.n_lm) + 1023) / 1024));
    hipLaunchKernelGGL(k_ba_gather_B, dim3(gb, 1, (unsigned)B.m.size()), dim3(256), 0, s, (const BADev *)B.d_arr);
    OV2_HIP_CHECK(hipGetLastError());
    uint8_t *hb = (uint8_t *)ctx->h_scratch, *db = (uint8_t *)ctx->d_scratch;
    OV2_HIP_CHECK(hipMemcpyAsync(hb + B.out_base, db + B.out_base, B.out_total, hipMemcpyDeviceToHost, s));
    OV2_HIP_CHECK(hipStreamSynchronize(s));
    for (size_t k = 0; k < B.m.size(); k++) {
        const BAMember &q = B.m[k];
        ov2_local_ba_result &ri = r[q.i];
        const BADev &D = q.dev->D;
        const BAOutLayout L = ba_out_layout(D.n_kf, D.n_lm, D.n_res, q.out_flags);
        const uint8_t *o = hb + B.out_base + q.out_off;
        const size_t nr = (size_t)D.n_res;
        if (ri.poses_out) memcpy(ri.poses_out, o + L.poses, 56 * (size_t)D.n_kf);
        if (ri.invdepth_out) memcpy(ri.invdepth_out, o + L.invdepth, 8 * (size_t)D.n_lm);
        if (ri.bad_obs && nr > 0) memcpy(ri.bad_obs, o + L.bad_obs, nr);
        if (ri.chi2_last_eval && nr > 0) memcpy(ri.chi2_last_eval, o + L.chi2, 8 * nr);
        if (ri.depthpos_last_eval && nr > 0) memcpy(ri.depthpos_last_eval, o + L.dpos, nr);
        local_ba_second_test(ri, B.h_cnt[16 * k]);
    }
    return OV2_OK;
}

// ov2_local_ba_batch behind its argument check: every problem is attempted, r[i].status says which results are valid, the call
// returns the first failure in problem order.  A step of the shared part that fails is the status of every member it left without
// a result (their buffers are not written); the problems that run alone still do
static int local_ba_batch(ov2_ctx *ctx, int n, const ov2_ba_problem *p, const ov2_local_ba_options *o, ov2_local_ba_result *r, int *n_batched)
{
    for (int i = 0; i < n; i++) local_ba_clear_result(r[i]);
    const int rc_all = local_ba_check_batch(ctx, n, o);
    if (rc_all != OV2_OK) {
        for (int i = 0; i < n; i++) r[i].status = rc_all;
        return rc_all;
    }
    std::vector<uint8_t> alone;
    {
        BABatch B;                                          // (gone before the problems that run alone reuse the context's blocks)
        B.m = local_ba_classify(ctx, n, p, r, alone);
        const BALap lap{"local_ba_batch", ctx->debug != 0};
        int rc = ba_batch_build(ctx, B, p, r, alone);
        lap("sort + upload (ba_create)");
        if (rc == OV2_OK && !B.m.empty()) {
            rc = local_ba_shared(ctx, B, o, r, lap);
            if (rc == OV2_OK) rc = ba_batch_fetch(ctx, B, r);
            lap("outlier test 2 + download");
        }
        if (n_batched) *n_batched = rc == OV2_OK ? (int)B.m.size() : 0;
        if (rc != OV2_OK) (void)hipStreamSynchronize(ctx->stream);            // (nothing of this batch may still be in flight)
        for (const BAMember &q : B.m) if (rc != OV2_OK) r[q.i].status = rc;
    }
    // what cannot share launches (large windows, pose-only blocks, the deterministic mode): one problem at a time
    for (int i = 0; i < n; i++) if (alone[(size_t)i]) (void)ov2_local_ba(ctx, &p[i], &o[i], &r[i]);
    for (int i = 0; i < n; i++) if (r[i].status != OV2_OK) return r[i].status;
    return OV2_OK;
}
