// monoinit.hip -- trackMono's un-initialised branch (src/visual_front_end.cpp:98-113) with VisualFrontEnd::checkReadyForInit
// (:855-984) for gfx950 as ONE device chain per call, on a block the caller owns (monoinit_dev.hpp).  include/ov2slam_hip.h states the
// semantics line by line; tests/monoinit_ref.py is the same in numpy.
//   k_fkf_parallax  fkf.hip, unchanged, in the form (unrot = 0, OV2_FKF_ALL, OV2_FKF_MEDIAN): p0 of :857.
//   k_minit_gather  ONE WORK-GROUP OF FOUR WAVEFRONTS PER ITEM.  All lanes: the 2-D keypoints counted by ballots (:100), the
//                   keyframe's ascending ids into LDS; the three early returns (:100, :861, :873) are uniform over the work-group and
//                   end it.  Then the join (fkf_find) and the rotation-compensated distance of :908-913 (minit_rot_dist: K as a
//                   matrix, NOT fkf_unrot_dist) of every current keypoint into LDS.  The FIRST WAVEFRONT does what has an order: it
//                   compacts the joined pairs by ballot-prefix into bv1 / bv2 / pair_cur (stable in array order), adds the distances
//                   64 at a time in lane order into the serial widened float sum (fkf_wide_add64), evaluates :917 and :925 and
//                   writes the E5Item of the search -- n = 0, S = 0 for an item that returned early, so the search kernels skip it.
//                   Where the item searches, all lanes draw the sample table (epif_draw_table, the draw of k_epif_gather).
//   k_e5_solve, k_e5_score, k_e5_pick   fivept.hip, unchanged, through e5_enqueue.
//   k_minit_decide  ONE WAVEFRONT PER ITEM.  The NO_MODEL return, the removal flags through pair_cur (in LDS, so that every output
//                   byte is stored once), the initial pose, the output record.
//   k_minit_input, k_minit_apply   the lock-step form (ov2_btracker_mono_init, trackb_monoinit.hip): the chain's inputs from the
//                   resident frame, its results onto the resident frame, pose and motion state (monoinit_dev.hpp).
// No atomics in this file's kernels, no result that depends on scheduling.  Every count read from device memory is clamped before it
// indexes.
#include "monoinit_dev.hpp"
#include "epif_dev.hpp"
#include <cmath>

#pragma clang fp contract(off)

struct MinitArgs {
    const FkfItemD *fi; const MinitItem *mi; const int *fo;
    const int *cur_lmid; const double *cur_bv; const uint8_t *cur_is3d;
    const int *kf_lmid; const float2 *kf_unpx; const double *kf_bv;
    double *bv1, *bv2; int *pair_cur; E5Item *e5; int4 *samples;
    const E5Out *e5out; const int *outliers;
    MinitOut *out; uint8_t *removed;
    double K[4];
    float finit_parallax;
    int min_2d_kps;
};

// :908-913: cv::norm(Point2f(u.x / u.z, u.y / u.z) - kf_unpx), u = K (R bv) with K a full 3 x 3 matrix (its zeros take part: 0 * x is
// -0 or NaN for some x, and the header promises the reference's coefficients, not a simplification of them)
__device__ __forceinline__ double minit_rot_dist(const double K[4], const double R[9], const double *bv, float2 kf_unpx)
{
    const TriD3 r = tri_matvec(R, TriD3{bv[0], bv[1], bv[2]});
    const double ux = (K[0] * r.x + 0. * r.y) + K[2] * r.z;
    const double uy = (0. * r.x + K[1] * r.y) + K[3] * r.z;
    const double uz = (0. * r.x + 0. * r.y) + 1. * r.z;
    return tri_pdist(make_float2((float)(ux / uz), (float)(uy / uz)), kf_unpx);
}

__global__ __launch_bounds__(EPIF_THREADS) void k_minit_gather(MinitArgs a)
{
    __shared__ double s_d[OV2_FKF_MAX_POINTS];                     // the distance of current keypoint i, +0 without a counterpart
    __shared__ int s_k[OV2_FKF_MAX_POINTS];                        // the keyframe's ids; afterwards the draw's window
    __shared__ short s_j[OV2_FKF_MAX_POINTS];                      // the keyframe slot of current keypoint i, -1: none
    __shared__ unsigned short s_start[EPIF_WIN / 8];
    __shared__ int s_ctl[8];                                       // per-wavefront 2-D counts [0, 4), m, S
    static_assert(2 * EPIF_WIN * sizeof(unsigned short) <= sizeof(int) * OV2_FKF_MAX_POINTS, "the window fits over the ids");
    static_assert(3 * EPIF_WIN * sizeof(unsigned short) <= sizeof(double) * OV2_FKF_MAX_POINTS, "the counts fit over the distances");
    const FkfItemD &it = a.fi[blockIdx.x];
    const MinitItem &mi = a.mi[blockIdx.x];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int n_cur = epif_clamp(it.n_cur, 0, OV2_FKF_MAX_POINTS), n_kf = epif_clamp(it.n_kf, 0, OV2_FKF_MAX_POINTS);
    const size_t c0 = (size_t)it.cur0, k0 = (size_t)it.kf0;
    for (int i = t; i < n_kf; i += EPIF_THREADS) s_k[i] = a.kf_lmid[k0 + i];
    int cnt = 0;                                                   // :100
    for (int base = 64 * wave; base < n_cur; base += EPIF_THREADS) {
        const int i = base + lane;
        cnt += __popcll(__ballot(i < n_cur && a.cur_is3d[c0 + i] == 0));
    }
    if (lane == 0) s_ctl[wave] = cnt;
    __syncthreads();
    const int nb2d = (s_ctl[0] + s_ctl[1]) + (s_ctl[2] + s_ctl[3]);
    const int *fo = a.fo + FKF_OUT_INTS * (size_t)blockIdx.x;
    const float p0 = __int_as_float(fo[0]);
    const bool reset = nb2d < a.min_2d_kps;                                            // :100
    const bool low = !((double)p0 > (double)a.finit_parallax);                         // :861, fails for NaN
    const bool too_few = it.n_cur < 8;                                                 // :873
    if (reset || low || too_few) {                                 // uniform: the whole work-group leaves
        if (t == 0) {
            a.e5[blockIdx.x] = E5Item{0, 0, it.cur0, mi.row0};
            MinitOut &o = a.out[blockIdx.x];
            o.action = reset ? OV2_MINIT_RESET : (low ? OV2_MINIT_LOW_PARALLAX : OV2_MINIT_TOO_FEW_KPS);
            o.nb2dkps = nb2d;
            o.p0 = reset ? 0.f : p0; o.p0_n = reset ? 0 : fo[1]; o.p0_n_distinct = reset ? 0 : fo[2]; o.p0_n_nonfinite = reset ? 0 : fo[3];
            o.m = 0; o.p1 = 0.f; o.searched = 0;
        }
        return;
    }
    double R[9];
    fkf_rkfcur(it.kf_Tcw, it.cur_Twc, R);                          // :887
    for (int i = t; i < n_cur; i += EPIF_THREADS) {                // :893-913 per keypoint: the join and the distance, by all lanes
        const int j = fkf_find(s_k, n_kf, a.cur_lmid[c0 + i]);
        s_j[i] = (short)j;
        s_d[i] = j >= 0 ? minit_rot_dist(a.K, R, a.cur_bv + 3 * (c0 + (size_t)i), a.kf_unpx[k0 + (size_t)j]) : 0.;
    }
    __syncthreads();
    if (wave == 0) {                                               // what has an order: the compaction and the sum, in array order
        int m = 0;
        float sum = 0.f;
        for (int base = 0; base < n_cur; base += 64) {
            const int i = base + lane;
            const int j = i < n_cur ? s_j[i] : -1;
            const unsigned long long mask = __ballot(j >= 0);
            if (mask == 0ull) continue;
            if (j >= 0) {
                const double *cb = a.cur_bv + 3 * (c0 + (size_t)i), *kb = a.kf_bv + 3 * (k0 + (size_t)j);
                const size_t pos = c0 + (size_t)(m + __popcll(mask & ((1ull << lane) - 1ull)));
                a.bv1[3 * pos] = kb[0]; a.bv1[3 * pos + 1] = kb[1]; a.bv1[3 * pos + 2] = kb[2];
                a.bv2[3 * pos] = cb[0]; a.bv2[3 * pos + 1] = cb[1]; a.bv2[3 * pos + 2] = cb[2];
                a.pair_cur[pos] = i;
            }
            sum = fkf_wide_add64(sum, i < n_cur ? s_d[i] : 0.);    // :913; a lane without a match adds +0: no bit of the sum changes
            m += __popcll(mask);
        }
        const bool few_matches = m < 8;                                               // :917
        const float p1 = few_matches ? 0.f : sum / (float)m;                          // :923
        const bool low_rot = !few_matches && p1 < a.finit_parallax;                   // :925, false for NaN
        const bool reached = !few_matches && !low_rot;                                // the reference calls the search
        const int S = reached ? epif_clamp(mi.n_rows, 0, OV2_EPI_MAX_ROWS) : 0;
        if (lane == 0) {
            a.e5[blockIdx.x] = E5Item{reached ? m : 0, S, it.cur0, mi.row0};
            MinitOut &o = a.out[blockIdx.x];
            o.action = few_matches ? OV2_MINIT_TOO_FEW_MATCHES : (low_rot ? OV2_MINIT_LOW_ROT_PARALLAX : OV2_MINIT_NO_MODEL);
            o.nb2dkps = nb2d;
            o.p0 = p0; o.p0_n = fo[1]; o.p0_n_distinct = fo[2]; o.p0_n_nonfinite = fo[3];
            o.m = m; o.p1 = p1; o.searched = reached ? 1 : 0;
            s_ctl[4] = m; s_ctl[5] = S;
        }
    }
    __syncthreads();
    const int m = s_ctl[4], S = s_ctl[5];
    if (S == 0) return;
    // the distances and the ids are done with: the draw's windows go over them (epif_draw_table, epif_dev.hpp)
    epif_draw_table(mi.seed, m, S, a.samples + 2 * (size_t)mi.row0, (unsigned short *)s_k, (unsigned short *)s_d, s_start, t);
}

// :968-973 from the unrefined model: [0.25 tkfc / |tkfc|, q(Rkfc)], the normalisation as epif_mono_pose's
__device__ __forceinline__ void minit_pose(const double *model, double *Twc)
{
    const double nt = sqrt((model[9] * model[9] + model[10] * model[10]) + model[11] * model[11]);
    const double ux = model[9] / nt, uy = model[10] / nt, uz = model[11] / nt;       // tkfc.normalize()
    double p[7];
    pose_from_model(model, p);                                                        // setRotationMatrix(Rkfc)
    Twc[0] = ux * 0.25; Twc[1] = uy * 0.25; Twc[2] = uz * 0.25;                       // tkfc.eval() * 0.25
    Twc[3] = p[3]; Twc[4] = p[4]; Twc[5] = p[5]; Twc[6] = p[6];
}

__global__ __launch_bounds__(64) void k_minit_decide(MinitArgs a)
{
    __shared__ uint8_t s_rm[OV2_FKF_MAX_POINTS];
    const FkfItemD &it = a.fi[blockIdx.x];
    MinitOut &o = a.out[blockIdx.x];
    const E5Out &e = a.e5out[blockIdx.x];
    const int lane = threadIdx.x;
    const int n_cur = epif_clamp(it.n_cur, 0, OV2_FKF_MAX_POINTS);
    const size_t c0 = (size_t)it.cur0;
    const int m = epif_clamp(o.m, 0, n_cur);
    const bool reached = o.searched != 0;
    for (int i = lane; i < n_cur; i += 64) s_rm[i] = 0;
    __syncthreads();
    int action = o.action, n_out = 0, n_rm = 0;
    double Twc[7] = {0., 0., 0., 0., 0., 0., 0.}, model[12];
#pragma unroll
    for (int q = 0; q < 12; q++) model[q] = reached ? e.model[q] : 0.;
    if (reached) {
        n_out = epif_clamp(e.n_outliers, 0, m);
        if (e.status != 0) action = OV2_MINIT_NO_MODEL;                               // :956
        else {
            action = OV2_MINIT_READY;
            for (int k = lane; k < n_out; k += 64) {                                  // :962-965; no 50 % rule
                const int idx = a.outliers[c0 + (size_t)k];
                if ((unsigned)idx < (unsigned)m) {
                    const int pc = a.pair_cur[c0 + (size_t)idx];
                    if ((unsigned)pc < (unsigned)n_cur) s_rm[pc] = 1;
                }
            }
            n_rm = n_out;
            minit_pose(model, Twc);                                                   // :968-973
        }
    }
    __syncthreads();
    for (int i = lane; i < n_cur; i += 64) a.removed[c0 + (size_t)i] = s_rm[i];
    if (lane != 0) return;
#pragma unroll
    for (int q = 0; q < 12; q++) o.model[q] = model[q];
#pragma unroll
    for (int q = 0; q < 7; q++) o.Twc_init[q] = Twc[q];
    o.score = reached ? e.score : 0.;
    o.action = action; o.m = m;
    o.status = reached ? e.status : 0; o.best_row = reached ? e.best_row : -1;
    o.iterations = reached ? e.iterations : 0; o.rows_consumed = reached ? e.rows_consumed : 0;
    o.n_inliers = reached ? e.n_inliers : 0; o.n_outliers = n_out;
    o.n_removed = n_rm;
}

// ---- the lock-step form: the chain's inputs from the resident frame, its results onto the resident state ---------------------------
__global__ __launch_bounds__(RES_THREADS) void k_minit_input(MinitTrackArgs a)
{
    const int b = blockIdx.y, i = blockIdx.x * RES_THREADS + threadIdx.x;
    const int nm = a.n_max < OV2_FKF_MAX_POINTS ? a.n_max : OV2_FKF_MAX_POINTS;
    const size_t o = (size_t)b * (size_t)a.n_max;
    const bool on = a.act[b] != 0;
    int n = 0;
    ResItem src = ResItem();
    if (on) { src = res_item(a.f, b, 0); n = res_clamp(*src.n, nm); }
    if (i == 0) {
        a.nd[b] = n;
        FkfItemD &d = a.fi[b];
        d.cur0 = (int)o; d.n_cur = n; d.kf0 = (int)o; d.n_kf = on ? res_clamp(a.hdr[b].n_kf, nm) : 0;
        d.cur_id = 0; d.kf_id = 0; d.kf_nb3dkps = 0; d.localba_is_on = 0; d.noccupcells = 0; d.nb3dkps = 0; d.pad0 = 0; d.pad1 = 0;
        d.cur_time = 0.; d.kf_time = 0.;
#pragma unroll
        for (int c = 0; c < 7; c++) {
            d.cur_Twc[c] = on ? a.r_T[7 * (size_t)b + c] : (c == 6 ? 1. : 0.);
            d.kf_Tcw[c] = on ? a.hdr[b].kf_Tcw[c] : (c == 6 ? 1. : 0.);
        }
        a.mi[b] = MinitItem{b * a.n_rows, a.n_rows, on ? a.seed[b] : 0ull};
    }
    if (i >= n) return;
    a.px[o + i] = src.px[i];
    a.cur_lmid[o + i] = src.lmid[i];
    a.cur_is3d[o + i] = src.is3d[i];
}

__global__ __launch_bounds__(RES_THREADS) void k_minit_apply(MinitTrackArgs a)
{
    __shared__ int s_w[2][RES_WAVES];
    const int b = blockIdx.x, t = threadIdx.x;
    if (!a.act[b]) return;
    const int nm = a.n_max < OV2_FKF_MAX_POINTS ? a.n_max : OV2_FKF_MAX_POINTS;
    const size_t o = (size_t)b * (size_t)a.n_max;
    const ResItem src = res_item(a.f, b, 0), dst = res_item(a.f, b, 1);
    const int n = res_clamp(*src.n, nm);
    const MinitOut &q = a.out[b];
    const bool ready = q.action == OV2_MINIT_READY;                         // (work-group uniform)
    static_assert(sizeof(MinitOut) % 4 == 0 && sizeof(MinitOut) / 4 <= RES_THREADS, "the record goes down as ints, one a lane");
    if (t < (int)(sizeof(MinitOut) / 4)) ((int *)(a.rec + b))[t] = ((const int *)&q)[t];
    for (int i = t; i < n; i += RES_THREADS) a.rm[o + i] = a.removed[o + i];
    if (ready) {                                                            // OV2_RES_REMOVE's rule: the rest close up in slot order
        int m = 0;
        for (int i0 = 0, round = 0; i0 < n; i0 += RES_THREADS, round++) {
            const int i = i0 + t;
            const bool keep = i < n && a.removed[o + i] == 0;
            int lm = 0; float2 px = make_float2(0.f, 0.f); double w0 = 0., w1 = 0., w2 = 0.; uint8_t d3 = 0;
            if (keep) { lm = src.lmid[i]; px = src.px[i]; d3 = (uint8_t)(src.is3d[i] != 0); w0 = src.wpt[3 * i]; w1 = src.wpt[3 * i + 1]; w2 = src.wpt[3 * i + 2]; }
            const int r = res_rank(keep, round, s_w, m);                    // r <= i < n_max
            if (keep) { dst.lmid[r] = lm; dst.px[r] = px; dst.is3d[r] = d3; dst.wpt[3 * r] = w0; dst.wpt[3 * r + 1] = w1; dst.wpt[3 * r + 2] = w2; }
        }
        if (t == 0) *dst.n = m;
        if (t < 7) a.r_T[7 * (size_t)b + t] = q.Twc_init[t];                // Frame::setTwc
    }
    if (t == 0) a.r_st[b].prev_time = -1.;                                  // MotionModel::reset(): prevTwc_ stays
    if (t < 6) a.r_st[b].log_relT[t] = 0.;
}

int ov2_launch_minit_input(hipStream_t s, const MinitTrackArgs &a, int n_active)
{
    hipLaunchKernelGGL(k_minit_input, dim3((a.n_max + RES_THREADS - 1) / RES_THREADS, n_active), dim3(RES_THREADS), 0, s, a);
    OV2_HIP_CHECK(hipGetLastError());
    return OV2_OK;
}

int ov2_launch_minit_apply(hipStream_t s, const MinitTrackArgs &a, int n_active)
{
    hipLaunchKernelGGL(k_minit_apply, dim3(n_active), dim3(RES_THREADS), 0, s, a);
    OV2_HIP_CHECK(hipGetLastError());
    return OV2_OK;
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------
void minit_layout(size_t n_items, size_t NC, size_t NK, size_t NR, int s_max, MinitLayout *L)
{
    L->B = n_items; L->NC = NC; L->NK = NK; L->NR = NR; L->s_max = s_max;
    StageCursor c(16);
    L->o_fi = c.take(sizeof(FkfItemD) * n_items); L->o_mi = c.take(sizeof(MinitItem) * n_items);
    L->o_lm = c.take(4 * NC); L->o_un = c.take(8 * NC); L->o_bv = c.take(24 * NC); L->o_3d = c.take(NC);
    L->o_kl = c.take(4 * NK); L->o_ku = c.take(8 * NK); L->o_kb = c.take(24 * NK);
    L->o_up = L->o_fo = c.take(4 * FKF_OUT_INTS * n_items); L->o_b1 = c.take(24 * NC); L->o_b2 = c.take(24 * NC); L->o_ol = c.take(4 * NC);
    L->o_e5 = c.take(sizeof(E5Item) * n_items); L->o_eo = c.take(sizeof(E5Out) * n_items);
    L->o_md = c.take(96 * NR); L->o_va = c.take(NR); L->o_sc = c.take(8 * NR);
    L->o_down = L->o_out = c.take(sizeof(MinitOut) * n_items); L->o_rm = c.take(NC); L->o_pc = c.take(4 * NC);
    L->o_sm = c.take(32 * NR); L->total = c.off;
}

int minit_layout_capacity(int n_items, int n_max, int n_rows, MinitLayout *L)
{
    OV2_REQUIRE(n_items >= 0 && n_items <= 65535, OV2_EINVAL, "item count outside [0, 65535]");
    OV2_REQUIRE(n_max >= 0 && n_max <= OV2_FKF_MAX_POINTS, OV2_EINVAL, "capacity: more than OV2_FKF_MAX_POINTS keypoints per item");
    OV2_REQUIRE(n_rows >= 0 && n_rows <= OV2_EPI_MAX_ROWS, OV2_EINVAL, "n_rows outside [0, OV2_EPI_MAX_ROWS]");
    const size_t NC = (size_t)n_items * (size_t)n_max, NR = (size_t)n_items * (size_t)n_rows;
    OV2_REQUIRE(NC <= 0x7fffffff && NR <= 0x7fffffff, OV2_EINVAL, "capacity: more than 2^31 - 1 keypoints or rows in one call");
    minit_layout((size_t)n_items, NC, NC, NR, n_rows, L);
    return OV2_OK;
}

int minit_check_params(const ov2_mono_init_params *params)
{
    OV2_REQUIRE(params, OV2_EINVAL, "NULL params");
    OV2_REQUIRE(!params->epi.boptimize, OV2_EINVAL, "boptimize is not provided: OpenGV's non-linear refinement has no device form");
    OV2_REQUIRE(params->epi.max_iterations >= 0, OV2_EINVAL, "max_iterations < 0");
    OV2_REQUIRE(std::isfinite(params->epi.threshold) && params->epi.threshold > 0.0, OV2_EINVAL, "threshold <= 0 or not finite");
    OV2_REQUIRE(params->epi.probability > 0.0 && params->epi.probability < 1.0, OV2_EINVAL, "probability outside (0, 1)");
    OV2_REQUIRE(params->n_rows >= 0 && params->n_rows <= OV2_EPI_MAX_ROWS, OV2_EINVAL, "n_rows outside [0, OV2_EPI_MAX_ROWS]");
    OV2_REQUIRE(params->min_2d_kps >= 0, OV2_EINVAL, "min_2d_kps < 0");
    OV2_REQUIRE(std::isfinite(params->fkf.finit_parallax), OV2_EINVAL, "finit_parallax not finite");
    for (int j = 0; j < 4; j++) OV2_REQUIRE(std::isfinite(params->fkf.K[j]), OV2_EINVAL, "K not finite");
    return OV2_OK;
}

int minit_chain_enqueue(hipStream_t s, const ov2_mono_init_params *params, const MinitLayout &L, uint8_t *ds, int n_items, const MinitKf *kf)
{
    if (n_items <= 0) return OV2_OK;
    MinitArgs a;
    a.fi = (const FkfItemD *)(ds + L.o_fi); a.mi = (const MinitItem *)(ds + L.o_mi); a.fo = (const int *)(ds + L.o_fo);
    a.cur_lmid = (const int *)(ds + L.o_lm); a.cur_bv = (const double *)(ds + L.o_bv); a.cur_is3d = ds + L.o_3d;
    a.kf_lmid = (const int *)(ds + L.o_kl); a.kf_unpx = (const float2 *)(ds + L.o_ku); a.kf_bv = (const double *)(ds + L.o_kb);
    if (kf) { a.kf_lmid = kf->lmid; a.kf_unpx = kf->unpx; a.kf_bv = kf->bv; }
    a.bv1 = (double *)(ds + L.o_b1); a.bv2 = (double *)(ds + L.o_b2); a.pair_cur = (int *)(ds + L.o_pc);
    a.e5 = (E5Item *)(ds + L.o_e5); a.samples = (int4 *)(ds + L.o_sm);
    a.e5out = (const E5Out *)(ds + L.o_eo); a.outliers = (const int *)(ds + L.o_ol);
    a.out = (MinitOut *)(ds + L.o_out); a.removed = ds + L.o_rm;
    for (int j = 0; j < 4; j++) a.K[j] = params->fkf.K[j];
    a.finit_parallax = params->fkf.finit_parallax; a.min_2d_kps = params->min_2d_kps;
    int rc = ov2_launch_parallax(s, &params->fkf, 0, OV2_FKF_ALL, OV2_FKF_MEDIAN, n_items, a.fi, a.cur_lmid, (const float2 *)(ds + L.o_un),
                                 a.cur_bv, a.cur_is3d, a.kf_lmid, a.kf_unpx, (int *)(ds + L.o_fo));       // :857
    if (rc) return rc;
    hipLaunchKernelGGL(k_minit_gather, dim3(n_items), dim3(EPIF_THREADS), 0, s, a);
    OV2_HIP_CHECK(hipGetLastError());
    E5Args e;
    e.items = a.e5; e.bv1 = a.bv1; e.bv2 = a.bv2; e.samples = a.samples;
    e.models = (double *)(ds + L.o_md); e.valid = ds + L.o_va; e.score = (double *)(ds + L.o_sc);
    e.out = (E5Out *)(ds + L.o_eo); e.outliers = (int *)(ds + L.o_ol);
    e.max_iterations = params->epi.max_iterations; e.threshold = params->epi.threshold; e.probability = params->epi.probability;
    rc = e5_enqueue(s, e, n_items, L.s_max);
    if (rc) return rc;
    hipLaunchKernelGGL(k_minit_decide, dim3(n_items), dim3(64), 0, s, a);
    OV2_HIP_CHECK(hipGetLastError());
    return OV2_OK;
}

void minit_record(const MinitOut &o, ov2_mono_init_result *r)
{
    r->action = o.action; r->nb2dkps = o.nb2dkps; r->p0 = o.p0; r->p0_n = o.p0_n; r->p0_n_distinct = o.p0_n_distinct;
    r->p0_n_nonfinite = o.p0_n_nonfinite; r->m = o.m; r->p1 = o.p1; r->status = o.status; r->best_row = o.best_row;
    r->iterations = o.iterations; r->rows_consumed = o.rows_consumed; r->score = o.score; r->n_inliers = o.n_inliers;
    r->n_outliers = o.n_outliers; r->n_removed = o.n_removed; r->pose_refined = 0;
    memcpy(r->model, o.model, sizeof o.model); memcpy(r->Twc_init, o.Twc_init, sizeof o.Twc_init);
}

static bool minit_finite(const double *p, size_t n)
{
    for (size_t i = 0; i < n; i++)
        if (!std::isfinite(p[i])) return false;
    return true;
}

int ov2_mono_init_batch(ov2_ctx *ctx, const ov2_mono_init_params *params, int n_items, const ov2_mono_init_item *items,
                        ov2_mono_init_result *results)
{
    // the inputs first, the context last: a malformed input is reported without a device
    int rc = minit_check_params(params);
    if (rc) return rc;
    OV2_REQUIRE(n_items >= 0, OV2_EINVAL, "n_items < 0");
    OV2_REQUIRE(n_items == 0 || (items && results), OV2_EINVAL, "NULL item / result array");
    OV2_REQUIRE(n_items <= 65535, OV2_EINVAL, "more than 65535 items in one call");
    size_t NC = 0, NK = 0;
    bool trace = false;
    for (int b = 0; b < n_items; b++) {
        const ov2_mono_init_item &k = items[b];
        const ov2_fkf_item &f = k.fkf;
        OV2_REQUIRE(f.n_cur >= 0 && f.n_kf >= 0, OV2_EINVAL, "negative count (n_cur / n_kf)");
        OV2_REQUIRE(f.n_cur <= OV2_FKF_MAX_POINTS && f.n_kf <= OV2_FKF_MAX_POINTS, OV2_EINVAL,
                    "more than OV2_FKF_MAX_POINTS (2048) keypoints in the frame or the keyframe");
        size_t n1 = 0, m1 = 0;
        int n_max = 0;
        rc = fkf_check_items(1, &f, true, &n1, &m1, &n_max);      // what ov2_parallax refuses (NULL arrays and poses, unsorted kf_lmid)
        if (rc) return rc;
        OV2_REQUIRE(f.n_kf == 0 || k.kf_bv, OV2_EINVAL, "NULL kf_bv");
        OV2_REQUIRE(f.n_cur == 0 || results[b].removed, OV2_EINVAL, "NULL result buffer (removed)");
        OV2_REQUIRE(minit_finite(f.cur_Twc, 7) && minit_finite(f.kf_Tcw, 7), OV2_EINVAL, "pose not finite (cur_Twc / kf_Tcw)");
        OV2_REQUIRE(minit_finite(f.cur_bv, 3 * (size_t)f.n_cur) && minit_finite(k.kf_bv, 3 * (size_t)f.n_kf), OV2_EINVAL,
                    "cur_bv / kf_bv not finite");
        trace = trace || results[b].trace_samples;
        NC += (size_t)f.n_cur; NK += (size_t)f.n_kf;
    }
    const size_t NR = (size_t)n_items * (size_t)params->n_rows;
    OV2_REQUIRE(NR <= 0x7fffffff, OV2_EINVAL, "capacity: more than 2^31 - 1 sample rows in one call");
    OV2_REQUIRE(ctx, OV2_EINVAL, "NULL context");
    if (n_items == 0) return OV2_OK;

    MinitLayout L;
    minit_layout((size_t)n_items, NC, NK, NR, params->n_rows, &L);
    const size_t down_end = trace ? L.total : L.o_sm;
    Stage st;
    rc = st.open(ctx, L.total, L.o_up > down_end - L.o_down ? L.o_up : down_end - L.o_down);  if (rc) return rc;
    uint8_t *hs = st.h, *ds = st.d;
    size_t p0 = 0, m0 = 0;
    for (int b = 0; b < n_items; b++) {
        const ov2_mono_init_item &k = items[b];
        const ov2_fkf_item &f = k.fkf;
        const size_t n = (size_t)f.n_cur, m = (size_t)f.n_kf;
        FkfItemD d;
        memset(&d, 0, sizeof d);
        d.cur0 = (int)p0; d.n_cur = f.n_cur; d.kf0 = (int)m0; d.n_kf = f.n_kf;
        memcpy(d.cur_Twc, f.cur_Twc, 56); memcpy(d.kf_Tcw, f.kf_Tcw, 56);
        memcpy(hs + L.o_fi + sizeof(FkfItemD) * b, &d, sizeof d);
        const MinitItem mi{b * params->n_rows, params->n_rows, k.seed};
        memcpy(hs + L.o_mi + sizeof(MinitItem) * b, &mi, sizeof mi);
        if (n) {
            memcpy(hs + L.o_lm + 4 * p0, f.cur_lmid, 4 * n);
            memcpy(hs + L.o_un + 8 * p0, f.cur_unpx, 8 * n);
            memcpy(hs + L.o_bv + 24 * p0, f.cur_bv, 24 * n);
            memcpy(hs + L.o_3d + p0, f.cur_is3d, n);
        }
        if (m) {
            memcpy(hs + L.o_kl + 4 * m0, f.kf_lmid, 4 * m);
            memcpy(hs + L.o_ku + 8 * m0, f.kf_unpx, 8 * m);
            memcpy(hs + L.o_kb + 24 * m0, k.kf_bv, 24 * m);
        }
        p0 += n; m0 += m;
    }
    rc = st.upload(0, L.o_up);  if (rc) return rc;
    rc = minit_chain_enqueue(ctx->stream, params, L, ds, n_items);
    if (rc) return rc;
    // the staging buffer is free again once the upload has run: the results come down over it
    rc = st.download(L.o_down, down_end, 0);  if (rc) return rc;
    rc = st.sync();  if (rc) return rc;
    auto hd = [&](size_t off) { return (const uint8_t *)hs + (off - L.o_down); };   // where the block's byte `off` came down
    p0 = 0;
    for (int b = 0; b < n_items; b++) {
        const size_t n = (size_t)items[b].fkf.n_cur;
        ov2_mono_init_result &r = results[b];
        MinitOut o;
        memcpy(&o, hd(L.o_out + sizeof(MinitOut) * b), sizeof o);
        minit_record(o, &r);
        if (n) {
            memcpy(r.removed, hd(L.o_rm + p0), n);
            if (r.pair_cur && o.m > 0) memcpy(r.pair_cur, hd(L.o_pc + 4 * p0), 4 * (size_t)(o.m < (int)n ? o.m : (int)n));
        }
        if (r.trace_samples && o.searched && params->n_rows > 0)
            memcpy(r.trace_samples, hd(L.o_sm + 32 * (size_t)b * (size_t)params->n_rows), 32 * (size_t)params->n_rows);
        p0 += n;
    }
    return OV2_OK;
}

int ov2_mono_init(ov2_ctx *ctx, const ov2_mono_init_params *params, const ov2_mono_init_item *item, ov2_mono_init_result *result)
{
    OV2_REQUIRE(item && result, OV2_EINVAL, "NULL item / result");
    return ov2_mono_init_batch(ctx, params, 1, item, result);
}
