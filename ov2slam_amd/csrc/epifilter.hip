// epifilter.hip -- VisualFrontEnd::epipolar2d2dFiltering (src/visual_front_end.cpp:440-656) for gfx950 as ONE device chain per
// call, on a block the caller owns (epif_dev.hpp).  include/ov2slam_hip.h states the semantics line by line; tests/epifilter_ref.py
// is the same in numpy.
//   k_epif_gather   ONE WORK-GROUP OF FOUR WAVEFRONTS PER ITEM.  All lanes: the keyframe's ascending ids into LDS, nb3dkps counted
//                   where asked, the join (fkf_find) and the rotation-compensated distance of every current keypoint into LDS.  The
//                   FIRST WAVEFRONT then does what has an order: it compacts the joined pairs by ballot-prefix into bv1 / bv2 /
//                   pair_cur (stable in array order), adds the distances 64 at a time in lane order into the serial widened float
//                   sum (fkf_wide_add64: the sum is serial by specification), evaluates the gate and writes the E5Item of the search
//                   -- n = 0, S = 0 for an item that returned early, so the search kernels skip it.  Where the item searches, all
//                   lanes draw the sample table.  A row starts from an empty state, so the number of draws consumed by "the row
//                   that starts at stream position p" depends on p alone: a window of 2048 positions goes to LDS (splitmix64 and
//                   the modulo by lanes), every position gets its count by lanes, the row starts follow as a chain of dependent
//                   LDS reads (the only serial part: one read per eight rows), and the rows are filled by lanes.  Every loop is bounded.
//                   (Measured on the way: one wavefront walking the stream draw by draw took 0.45 ms for 200 rows, as long as the
//                   search itself; the windowed draw in one wavefront 0.12 ms for the whole kernel.)
//   k_e5_solve, k_e5_score, k_e5_pick   fivept.hip, unchanged, through e5_enqueue.
//   k_epif_decide   ONE WAVEFRONT PER ITEM.  The NO_MODEL and DEGENERATE returns, the removal flags through pair_cur (in LDS, so
//                   that every output byte is stored once), the mono pose, F, the Sampson pass by lanes over the keypoints with ballot
//                   counts, the output record.
// No atomics, no result that depends on scheduling.  Every count read from device memory is clamped before it indexes.
#include "epif_dev.hpp"
#include "fkf_dev.hpp"
#include <cmath>

#pragma clang fp contract(off)

struct EpifArgs {
    const EpifItem *items;
    const int *cur_lmid; const float2 *cur_unpx; const double *cur_bv; const uint8_t *cur_is3d;
    const int *kf_lmid; const float2 *kf_unpx; const double *kf_bv;
    double *bv1, *bv2; int *pair_cur; E5Item *e5; int4 *samples;
    const E5Out *e5out; const int *outliers;
    EpifOut *out; uint8_t *removed; float *err;
    double K[4];
    int stereo, mono;
    float fransac_err;
};

__global__ __launch_bounds__(EPIF_THREADS) void k_epif_gather(EpifArgs a)
{
    __shared__ double s_d[OV2_FKF_MAX_POINTS];                     // the distance of current keypoint i, +0 without a counterpart
    __shared__ int s_k[OV2_FKF_MAX_POINTS];                        // the keyframe's ids; afterwards the draw's window
    __shared__ short s_j[OV2_FKF_MAX_POINTS];                      // the keyframe slot of current keypoint i, -1: none
    __shared__ unsigned short s_start[EPIF_WIN / 8];
    __shared__ int s_ctl[8];                                       // per-wavefront 3-D counts [0, 4), m, S
    static_assert(2 * EPIF_WIN * sizeof(unsigned short) <= sizeof(int) * OV2_FKF_MAX_POINTS, "the window fits over the ids");
    static_assert(3 * EPIF_WIN * sizeof(unsigned short) <= sizeof(double) * OV2_FKF_MAX_POINTS, "the counts fit over the distances");
    const EpifItem &it = a.items[blockIdx.x];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int n_cur = epif_clamp(it.n_cur, 0, OV2_FKF_MAX_POINTS), n_kf = epif_clamp(it.n_kf, 0, OV2_FKF_MAX_POINTS);
    const size_t c0 = (size_t)it.cur0, k0 = (size_t)it.kf0;
    for (int i = t; i < n_kf; i += EPIF_THREADS) s_k[i] = a.kf_lmid[k0 + i];
    int nb3d = it.nb3dkps;
    if (nb3d < 0) {                                                // pcurframe_->nb3dkps_ counted from the flags
        int cnt = 0;
        for (int base = 64 * wave; base < n_cur; base += EPIF_THREADS) {
            const int i = base + lane;
            cnt += __popcll(__ballot(i < n_cur && a.cur_is3d[c0 + i] != 0));
        }
        if (lane == 0) s_ctl[wave] = cnt;
    }
    __syncthreads();
    if (nb3d < 0) nb3d = (s_ctl[0] + s_ctl[1]) + (s_ctl[2] + s_ctl[3]);
    const bool from3d = a.stereo && nb3d > 30;                     // :484
    double R[9];
    fkf_rkfcur(it.kf_Tcw, it.cur_Twc, R);                          // :489
    for (int i = t; i < n_cur; i += EPIF_THREADS) {                // :492-517 per keypoint: the join and the distance, by all lanes
        int j = -1;
        if (!(from3d && a.cur_is3d[c0 + i] == 0)) j = fkf_find(s_k, n_kf, a.cur_lmid[c0 + i]);
        s_j[i] = (short)j;
        s_d[i] = j >= 0 ? fkf_unrot_dist(a.K, R, a.cur_bv + 3 * (c0 + (size_t)i), a.kf_unpx[k0 + (size_t)j]) : 0.;
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
            sum = fkf_wide_add64(sum, i < n_cur ? s_d[i] : 0.);    // :517; a lane without a match adds +0: no bit of the sum changes
            m += __popcll(mask);
        }
        const float par = m == 0 ? __int_as_float(0x7fc00000) : sum / (float)m;       // :528
        const bool too_few = it.n_cur < 8;                                            // :462
        const bool low = (double)par < 2. * (double)a.fransac_err;                    // :530, false for NaN
        const bool reached = !too_few && !low;                                        // the reference calls the search
        const int S = (reached && m >= 8) ? epif_clamp(it.n_rows, 0, OV2_EPI_MAX_ROWS) : 0;
        if (lane == 0) {
            a.e5[blockIdx.x] = E5Item{reached ? m : 0, S, it.cur0, it.row0};
            EpifOut &o = a.out[blockIdx.x];
            o.action = too_few ? OV2_EPIF_TOO_FEW_KPS : (low ? OV2_EPIF_LOW_PARALLAX : OV2_EPIF_NO_MODEL);
            o.m = m; o.epifrom3dkps = from3d ? 1 : 0;
            o.do_optimize = (a.mono && it.nbkfs > 2 && nb3d < 30) ? 1 : 0;            // :540
            o.nb3dkps = nb3d; o.parallax = par; o.searched = reached ? 1 : 0;
            s_ctl[4] = m; s_ctl[5] = S;
        }
    }
    __syncthreads();
    const int m = s_ctl[4], S = s_ctl[5];
    if (S == 0) return;
    // the distances and the ids are done with: the draw's windows go over them (epif_draw_table, epif_dev.hpp)
    epif_draw_table(it.seed, m, S, a.samples + 2 * (size_t)it.row0, (unsigned short *)s_k, (unsigned short *)s_d, s_start, t);
}

// C = A B, full 3 x 3 products, each sum of three terms serial
__device__ __forceinline__ void epif_mul33(const double *A, const double *B, double *C)
{
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) C[3 * r + c] = (A[3 * r] * B[c] + A[3 * r + 1] * B[3 + c]) + A[3 * r + 2] * B[6 + c];
}

// computeFundamentalMat12(identity, SE3(Rkfc, tkfc), K), src/multi_view_geometry.cpp:824-832: K^-T hat(t) R' K^-1, left to right
__device__ __forceinline__ void epif_fundamental(const double K[4], const double *model, double *F)
{
    double p[7], Rq[9], A[9], B[9];
    pose_from_model(model, p);                                     // Sophus::SE3d(Rkfc, tkfc): the quaternion of Rkfc ...
    tri_rotmat(TriQ{p[3], p[4], p[5], p[6]}, Rq);                  // ... and T12.rotationMatrix() back from it
    const double ix = 1. / K[0], iy = 1. / K[1], mx = -K[2] / K[0], my = -K[3] / K[1];
    const double iK[9] = {ix, 0., mx, 0., iy, my, 0., 0., 1.}, iKt[9] = {ix, 0., 0., 0., iy, 0., mx, my, 1.};
    const double tx = model[9], ty = model[10], tz = model[11];
    const double hat[9] = {0., -tz, ty, tz, 0., -tx, -ty, tx, 0.};
    epif_mul33(iKt, hat, A);
    epif_mul33(A, Rq, B);
    epif_mul33(B, iK, F);
}

// :594-607 from the unrefined model: kf_Twc * SE3(Rkfc, scale * tkfc / |tkfc|), scale = |(kf_Tcw * cur_Twc).translation()|
__device__ __forceinline__ void epif_mono_pose(const EpifItem &it, const double *model, double *Twc)
{
    const TriSE3 Tkfcur = tri_mul(tri_load(it.kf_Tcw), tri_load(it.cur_Twc));
    const double scale = sqrt(tri_dot(Tkfcur.t, Tkfcur.t));
    const double nt = sqrt((model[9] * model[9] + model[10] * model[10]) + model[11] * model[11]);
    const double ux = model[9] / nt, uy = model[10] / nt, uz = model[11] / nt;       // tkfc.normalize()
    double p[7];
    pose_from_model(model, p);
    const TriSE3 Tkfc{TriD3{scale * ux, scale * uy, scale * uz}, TriQ{p[3], p[4], p[5], p[6]}};
    const TriSE3 T = tri_mul(tri_load(it.kf_Twc), Tkfc);
    Twc[0] = T.t.x; Twc[1] = T.t.y; Twc[2] = T.t.z; Twc[3] = T.q.x; Twc[4] = T.q.y; Twc[5] = T.q.z; Twc[6] = T.q.w;
}

__global__ __launch_bounds__(64) void k_epif_decide(EpifArgs a)
{
    __shared__ uint8_t s_rm[OV2_FKF_MAX_POINTS];
    const EpifItem &it = a.items[blockIdx.x];
    EpifOut &o = a.out[blockIdx.x];
    const E5Out &e = a.e5out[blockIdx.x];
    const int lane = threadIdx.x;
    const int n_cur = epif_clamp(it.n_cur, 0, OV2_FKF_MAX_POINTS), n_kf = epif_clamp(it.n_kf, 0, OV2_FKF_MAX_POINTS);
    const size_t c0 = (size_t)it.cur0, k0 = (size_t)it.kf0;
    const int m = epif_clamp(o.m, 0, n_cur);
    const bool reached = o.searched != 0, from3d = o.epifrom3dkps != 0, do_opt = o.do_optimize != 0;
    for (int i = lane; i < n_cur; i += 64) s_rm[i] = 0;
    __syncthreads();
    int action = o.action, n_rr = 0, pfm = 0, n_out = 0;
    bool pass = false;
    double F[9] = {0., 0., 0., 0., 0., 0., 0., 0., 0.}, Twc[7] = {0., 0., 0., 0., 0., 0., 0.}, model[12];
#pragma unroll
    for (int q = 0; q < 12; q++) model[q] = reached ? e.model[q] : 0.;
    if (reached) {
        n_out = epif_clamp(e.n_outliers, 0, m);
        if (e.status != 0) action = OV2_EPIF_NO_MODEL;                                // :574
        else if ((double)n_out > 0.5 * (double)m) action = OV2_EPIF_DEGENERATE;       // :580
        else {
            action = OV2_EPIF_FILTERED;
            for (int k = lane; k < n_out; k += 64) {                                  // :587-590
                const int idx = a.outliers[c0 + (size_t)k];
                if ((unsigned)idx < (unsigned)m) {
                    const int pc = a.pair_cur[c0 + (size_t)idx];
                    if ((unsigned)pc < (unsigned)n_cur) s_rm[pc] = 1;
                }
            }
            n_rr = n_out;
            if (do_opt) { epif_mono_pose(it, model, Twc); pfm = 1; }                  // :594 (do_optimize holds nbkfs > 2)
            if (from3d) { epif_fundamental(a.K, model, F); pass = true; }             // :611-619
        }
    }
    __syncthreads();
    int n_rs = 0;
    for (int base = 0; base < n_cur; base += 64) {                                    // :624-648
        const int i = base + lane;
        const bool live = i < n_cur;
        int rm = 0;
        if (live) {
            const size_t g = c0 + (size_t)i;
            float er = 0.f;
            rm = s_rm[i];
            if (pass && a.cur_is3d[g] == 0) {
                const int j = fkf_find(a.kf_lmid + k0, n_kf, a.cur_lmid[g]);
                const float2 c = a.cur_unpx[g];
                const float2 kp = j >= 0 ? a.kf_unpx[k0 + (size_t)j] : make_float2(0.f, 0.f);   // Keypoint(): unpx_ = (0, 0), :633
                er = sampson(F, c.x, c.y, kp.x, kp.y);                                // :639
                if (er > a.fransac_err) rm = 2;                                       // :641
            }
            a.removed[g] = (uint8_t)rm;
            a.err[g] = er;
        }
        n_rs += __popcll(__ballot(live && rm == 2));
    }
    if (lane != 0) return;
#pragma unroll
    for (int q = 0; q < 12; q++) o.model[q] = model[q];
#pragma unroll
    for (int q = 0; q < 9; q++) o.F[q] = F[q];
#pragma unroll
    for (int q = 0; q < 7; q++) o.Twc_model[q] = Twc[q];
    o.score = reached ? e.score : 0.;
    o.action = action; o.m = m;
    o.status = reached ? e.status : 0; o.best_row = reached ? e.best_row : -1;
    o.iterations = reached ? e.iterations : 0; o.rows_consumed = reached ? e.rows_consumed : 0;
    o.n_inliers = reached ? e.n_inliers : 0; o.n_outliers = n_out;
    o.n_removed_ransac = n_rr; o.n_removed_sampson = n_rs; o.pose_from_model = pfm;
    o.pad[0] = 0; o.pad[1] = 0;
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------
void epif_layout(size_t n_items, size_t NC, size_t NK, size_t NR, int s_max, EpifLayout *L)
{
    L->B = n_items; L->NC = NC; L->NK = NK; L->NR = NR; L->s_max = s_max;
    StageCursor c(16);
    L->o_it = c.take(sizeof(EpifItem) * n_items); L->o_lm = c.take(4 * NC); L->o_un = c.take(8 * NC); L->o_bv = c.take(24 * NC);
    L->o_3d = c.take(NC); L->o_kl = c.take(4 * NK); L->o_ku = c.take(8 * NK); L->o_kb = c.take(24 * NK);
    L->o_up = L->o_b1 = c.take(24 * NC); L->o_b2 = c.take(24 * NC); L->o_ol = c.take(4 * NC); L->o_e5 = c.take(sizeof(E5Item) * n_items);
    L->o_eo = c.take(sizeof(E5Out) * n_items); L->o_md = c.take(96 * NR); L->o_va = c.take(NR); L->o_sc = c.take(8 * NR);
    L->o_down = L->o_out = c.take(sizeof(EpifOut) * n_items); L->o_rm = c.take(NC); L->o_pc = c.take(4 * NC); L->o_er = c.take(4 * NC);
    L->o_sm = c.take(32 * NR); L->total = c.off;
}

int epif_layout_capacity(int n_items, int n_max, int n_rows, EpifLayout *L)
{
    OV2_REQUIRE(n_items >= 0 && n_items <= 65535, OV2_EINVAL, "item count outside [0, 65535]");
    OV2_REQUIRE(n_max >= 0 && n_max <= OV2_FKF_MAX_POINTS, OV2_EINVAL, "capacity: more than OV2_FKF_MAX_POINTS keypoints per item");
    OV2_REQUIRE(n_rows >= 0 && n_rows <= OV2_EPI_MAX_ROWS, OV2_EINVAL, "n_rows outside [0, OV2_EPI_MAX_ROWS]");
    const size_t NC = (size_t)n_items * (size_t)n_max, NR = (size_t)n_items * (size_t)n_rows;
    OV2_REQUIRE(NC <= 0x7fffffff && NR <= 0x7fffffff, OV2_EINVAL, "capacity: more than 2^31 - 1 keypoints or rows in one call");
    epif_layout((size_t)n_items, NC, NC, NR, n_rows, L);
    return OV2_OK;
}

int epif_check_params(const ov2_epifilter_params *params)
{
    OV2_REQUIRE(params, OV2_EINVAL, "NULL params");
    OV2_REQUIRE(!params->epi.boptimize, OV2_EINVAL, "boptimize is not provided: OpenGV's non-linear refinement has no device form");
    OV2_REQUIRE(params->epi.max_iterations >= 0, OV2_EINVAL, "max_iterations < 0");
    OV2_REQUIRE(std::isfinite(params->epi.threshold) && params->epi.threshold > 0.0, OV2_EINVAL, "threshold <= 0 or not finite");
    OV2_REQUIRE(params->epi.probability > 0.0 && params->epi.probability < 1.0, OV2_EINVAL, "probability outside (0, 1)");
    OV2_REQUIRE(params->n_rows >= 0 && params->n_rows <= OV2_EPI_MAX_ROWS, OV2_EINVAL, "n_rows outside [0, OV2_EPI_MAX_ROWS]");
    for (int j = 0; j < 4; j++) OV2_REQUIRE(std::isfinite(params->fkf.K[j]), OV2_EINVAL, "K not finite");
    return OV2_OK;
}

int epif_chain_enqueue(hipStream_t s, const ov2_epifilter_params *params, const EpifLayout &L, uint8_t *ds, int n_items)
{
    if (n_items <= 0) return OV2_OK;
    EpifArgs a;
    a.items = (const EpifItem *)(ds + L.o_it);
    a.cur_lmid = (const int *)(ds + L.o_lm); a.cur_unpx = (const float2 *)(ds + L.o_un); a.cur_bv = (const double *)(ds + L.o_bv);
    a.cur_is3d = ds + L.o_3d; a.kf_lmid = (const int *)(ds + L.o_kl); a.kf_unpx = (const float2 *)(ds + L.o_ku);
    a.kf_bv = (const double *)(ds + L.o_kb);
    a.bv1 = (double *)(ds + L.o_b1); a.bv2 = (double *)(ds + L.o_b2); a.pair_cur = (int *)(ds + L.o_pc);
    a.e5 = (E5Item *)(ds + L.o_e5); a.samples = (int4 *)(ds + L.o_sm);
    a.e5out = (const E5Out *)(ds + L.o_eo); a.outliers = (const int *)(ds + L.o_ol);
    a.out = (EpifOut *)(ds + L.o_out); a.removed = ds + L.o_rm; a.err = (float *)(ds + L.o_er);
    for (int j = 0; j < 4; j++) a.K[j] = params->fkf.K[j];
    a.stereo = params->fkf.stereo ? 1 : 0; a.mono = params->mono ? 1 : 0; a.fransac_err = params->fransac_err;
    hipLaunchKernelGGL(k_epif_gather, dim3(n_items), dim3(EPIF_THREADS), 0, s, a);
    OV2_HIP_CHECK(hipGetLastError());
    E5Args e;
    e.items = a.e5; e.bv1 = a.bv1; e.bv2 = a.bv2; e.samples = a.samples;
    e.models = (double *)(ds + L.o_md); e.valid = ds + L.o_va; e.score = (double *)(ds + L.o_sc);
    e.out = (E5Out *)(ds + L.o_eo); e.outliers = (int *)(ds + L.o_ol);
    e.max_iterations = params->epi.max_iterations; e.threshold = params->epi.threshold; e.probability = params->epi.probability;
    const int rc = e5_enqueue(s, e, n_items, L.s_max);
    if (rc) return rc;
    hipLaunchKernelGGL(k_epif_decide, dim3(n_items), dim3(64), 0, s, a);
    OV2_HIP_CHECK(hipGetLastError());
    return OV2_OK;
}

static bool epif_finite(const double *p, size_t n)
{
    for (size_t i = 0; i < n; i++)
        if (!std::isfinite(p[i])) return false;
    return true;
}

int ov2_epipolar_filter_batch(ov2_ctx *ctx, const ov2_epifilter_params *params, int n_items, const ov2_epifilter_item *items,
                              ov2_epifilter_result *results)
{
    // the inputs first, the context last: a malformed input is reported without a device
    int rc = epif_check_params(params);
    if (rc) return rc;
    OV2_REQUIRE(n_items >= 0, OV2_EINVAL, "n_items < 0");
    OV2_REQUIRE(n_items == 0 || (items && results), OV2_EINVAL, "NULL item / result array");
    OV2_REQUIRE(n_items <= 65535, OV2_EINVAL, "more than 65535 items in one call");
    size_t NC = 0, NK = 0;
    bool trace = false;
    for (int b = 0; b < n_items; b++) {
        const ov2_epifilter_item &k = items[b];
        const ov2_fkf_item &f = k.fkf;
        OV2_REQUIRE(f.n_cur >= 0 && f.n_kf >= 0, OV2_EINVAL, "negative count (n_cur / n_kf)");
        OV2_REQUIRE(f.n_cur <= OV2_FKF_MAX_POINTS && f.n_kf <= OV2_FKF_MAX_POINTS, OV2_EINVAL,
                    "more than OV2_FKF_MAX_POINTS (2048) keypoints in the frame or the keyframe");
        int n_max = 0;
        rc = fkf_check_items(1, &f, true, &NC, &NK, &n_max);      // what ov2_parallax refuses (NULL arrays and poses, unsorted kf_lmid)
        if (rc) return rc;
        OV2_REQUIRE(f.n_kf == 0 || (k.kf_bv && k.kf_Twc), OV2_EINVAL, "NULL kf_bv / kf_Twc");
        OV2_REQUIRE(f.n_cur == 0 || results[b].removed, OV2_EINVAL, "NULL result buffer (removed)");
        OV2_REQUIRE(epif_finite(f.cur_Twc, 7) && epif_finite(f.kf_Tcw, 7) && (!k.kf_Twc || epif_finite(k.kf_Twc, 7)), OV2_EINVAL,
                    "pose not finite (cur_Twc / kf_Tcw / kf_Twc)");
        OV2_REQUIRE(epif_finite(f.cur_bv, 3 * (size_t)f.n_cur) && epif_finite(k.kf_bv, 3 * (size_t)f.n_kf), OV2_EINVAL,
                    "cur_bv / kf_bv not finite");
        trace = trace || results[b].trace_samples;
    }
    NC = NK = 0;
    int n_max = 0;
    for (int b = 0; b < n_items; b++) {
        NC += (size_t)items[b].fkf.n_cur; NK += (size_t)items[b].fkf.n_kf;
        n_max = items[b].fkf.n_cur > n_max ? items[b].fkf.n_cur : n_max;
        n_max = items[b].fkf.n_kf > n_max ? items[b].fkf.n_kf : n_max;
    }
    const size_t NR = (size_t)n_items * (size_t)params->n_rows;
    OV2_REQUIRE(NR <= 0x7fffffff, OV2_EINVAL, "capacity: more than 2^31 - 1 sample rows in one call");
    OV2_REQUIRE(ctx, OV2_EINVAL, "NULL context");
    if (n_items == 0) return OV2_OK;

    // packed to the items' real sizes, or (OV2_OPT_EPIF_CAPACITY, for tests) the capacity form a fused step will use: item b's
    // keypoint and keyframe slots at b * n_max
    const bool capacity = ctx->epif_capacity != 0;
    EpifLayout L;
    if (capacity) {
        rc = epif_layout_capacity(n_items, n_max, params->n_rows, &L);
        if (rc) return rc;
    } else epif_layout((size_t)n_items, NC, NK, NR, params->n_rows, &L);
    const size_t down_end = trace ? L.total : L.o_sm;
    Stage st;
    rc = st.open(ctx, L.total, L.o_up > down_end - L.o_down ? L.o_up : down_end - L.o_down);  if (rc) return rc;
    uint8_t *hs = st.h, *ds = st.d;
    size_t p0 = 0, m0 = 0;
    for (int b = 0; b < n_items; b++) {
        const ov2_epifilter_item &k = items[b];
        const ov2_fkf_item &f = k.fkf;
        const size_t n = (size_t)f.n_cur, m = (size_t)f.n_kf;
        if (capacity) p0 = m0 = (size_t)b * (size_t)n_max;
        EpifItem d;
        memset(&d, 0, sizeof d);
        d.cur0 = (int)p0; d.n_cur = f.n_cur; d.kf0 = (int)m0; d.n_kf = f.n_kf;
        d.row0 = b * params->n_rows; d.n_rows = params->n_rows; d.nb3dkps = f.nb3dkps; d.nbkfs = k.nbkfs; d.seed = k.seed;
        memcpy(d.cur_Twc, f.cur_Twc, 56); memcpy(d.kf_Tcw, f.kf_Tcw, 56);
        if (k.kf_Twc) memcpy(d.kf_Twc, k.kf_Twc, 56);
        memcpy(hs + L.o_it + sizeof(EpifItem) * b, &d, sizeof d);
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
    rc = epif_chain_enqueue(ctx->stream, params, L, ds, n_items);
    if (rc) return rc;
    // the staging buffer is free again once the upload has run: the results come down over it
    rc = st.download(L.o_down, down_end, 0);  if (rc) return rc;
    rc = st.sync();  if (rc) return rc;
    auto hd = [&](size_t off) { return (const uint8_t *)hs + (off - L.o_down); };   // where the block's byte `off` came down
    p0 = 0;
    for (int b = 0; b < n_items; b++) {
        const size_t n = (size_t)items[b].fkf.n_cur;
        if (capacity) p0 = (size_t)b * (size_t)n_max;
        ov2_epifilter_result &r = results[b];
        EpifOut o;
        memcpy(&o, hd(L.o_out + sizeof(EpifOut) * b), sizeof o);
        r.action = o.action; r.m = o.m; r.epifrom3dkps = o.epifrom3dkps; r.do_optimize = o.do_optimize; r.nb3dkps = o.nb3dkps;
        r.parallax = o.parallax; r.status = o.status; r.best_row = o.best_row; r.iterations = o.iterations;
        r.rows_consumed = o.rows_consumed; r.score = o.score; r.n_inliers = o.n_inliers; r.n_outliers = o.n_outliers;
        memcpy(r.model, o.model, sizeof o.model); memcpy(r.F, o.F, sizeof o.F); memcpy(r.Twc_model, o.Twc_model, sizeof o.Twc_model);
        r.n_removed_ransac = o.n_removed_ransac; r.n_removed_sampson = o.n_removed_sampson; r.pose_from_model = o.pose_from_model;
        if (n) {
            memcpy(r.removed, hd(L.o_rm + p0), n);
            if (r.pair_cur && o.m > 0) memcpy(r.pair_cur, hd(L.o_pc + 4 * p0), 4 * (size_t)(o.m < (int)n ? o.m : (int)n));
            if (r.err) memcpy(r.err, hd(L.o_er + 4 * p0), 4 * n);
        }
        if (r.trace_samples && o.searched && o.m >= 8 && params->n_rows > 0)
            memcpy(r.trace_samples, hd(L.o_sm + 32 * (size_t)b * (size_t)params->n_rows), 32 * (size_t)params->n_rows);
        p0 += n;
    }
    return OV2_OK;
}

int ov2_epipolar_filter(ov2_ctx *ctx, const ov2_epifilter_params *params, const ov2_epifilter_item *item, ov2_epifilter_result *result)
{
    OV2_REQUIRE(item && result, OV2_EINVAL, "NULL item / result");
    return ov2_epipolar_filter_batch(ctx, params, 1, item, result);
}
