// fkf.hip -- "frame versus keyframe": the per-frame keypoint passes of the reference's src/visual_front_end.cpp for gfx950:
//   k_fkf_parallax   VisualFrontEnd::computeParallax (:1066-1141) in the arithmetic of its three call sites (:1003 rotation-
//                    compensated median, :857 plain average, :488-535 the wide accumulation ahead of the 5-point search) and, for
//                    ov2_kf_decision, the rule of VisualFrontEnd::checkNewKfReq (:986-1061) with the occupied-cell and 3-D counts.
//                    ONE WORK-GROUP PER ITEM: the join (Frame::getKeypointById as a binary search of the keyframe's ascending ids,
//                    staged in LDS), the per-keypoint arithmetic in fp64, one wavefront adding the distances in array order (the
//                    reference's float sum is serial; no tree), and the std::set<float> median over at most 2048 floats in LDS:
//                    bitonic sort padded with +inf, run heads flagged, scanned, the head of rank n_distinct / 2 picked.
//   k_fkf_sampson    the Sampson pass over the 2-D keypoints after the 5-point search (:610-652), one lane per keypoint.
// include/ov2slam_hip.h states the arithmetic; tests/kfreq_ref.py is the same in numpy.
#include "fkf_dev.hpp"                 // the join, the rotation, the distance and the widened sum: epifilter.hip uses them too

#pragma clang fp contract(off)

#define FKF_THREADS 256
#define FKF_INF_BITS 0x7f800000

// FkfParamsD, FkfItemD, FKF_OUT_INTS: fkf_dev.hpp (the lock-step step fills the item records on the device)

__global__ __launch_bounds__(FKF_THREADS) void k_fkf_parallax(FkfParamsD P, const FkfItemD *__restrict__ items, const int *__restrict__ cur_lmid,
                                                              const float2 *__restrict__ cur_px, const float2 *__restrict__ cur_unpx,
                                                              const double *__restrict__ cur_bv, const uint8_t *__restrict__ cur_is3d,
                                                              const int *__restrict__ kf_lmid, const float2 *__restrict__ kf_unpx,
                                                              int *__restrict__ out)
{
    __shared__ double s_d[OV2_FKF_MAX_POINTS];          // d per current keypoint, -1: not in the statistic
    __shared__ int s_k[OV2_FKF_MAX_POINTS];             // the keyframe's ids, then the sort keys (bits of p >= +0: integer order is float order)
    __shared__ unsigned s_bm[OV2_FKF_MAX_CELLS / 32];   // occupied cells
    __shared__ int s_cnt[8];                            // n, n_nonfinite, nb3dkps, n_out_of_grid, noccupcells
    __shared__ int s_wave[FKF_THREADS / 64];
    __shared__ float s_sum, s_med;
    const FkfItemD &it = items[blockIdx.x];
    const int t = threadIdx.x, n_cur = it.n_cur, n_kf = it.n_kf, cur0 = it.cur0, kf0 = it.kf0;
    const bool count_cells = P.decide && it.noccupcells < 0, count_3d = P.decide && it.nb3dkps < 0;
    const int ncells = P.nbwcells * P.nbhcells, nwords = (ncells + 31) >> 5;     // <= OV2_FKF_MAX_CELLS, checked by the host

    for (int i = t; i < n_kf; i += FKF_THREADS) s_k[i] = kf_lmid[kf0 + i];
    if (count_cells)
        for (int w = t; w < nwords; w += FKF_THREADS) s_bm[w] = 0u;
    if (t < 8) s_cnt[t] = 0;
    __syncthreads();

    double R[9] = {1., 0., 0., 0., 1., 0., 0., 0., 1.};
    if (P.unrot) fkf_rkfcur(it.kf_Tcw, it.cur_Twc, R);  // Rkfcur = Rkfw * Rwcur, :1082-1084
    int my_n = 0, my_nf = 0, my_3d = 0, my_oog = 0;
    for (int i = t; i < n_cur; i += FKF_THREADS) {
        const int g = cur0 + i;
        const bool is3d = cur_is3d[g] != 0;
        if (count_3d) my_3d += is3d ? 1 : 0;
        if (count_cells) {                              // Frame::getKeypointCellIdx, frame.cpp:587-592
            const float2 px = cur_px[g];
            const float rf = floorf(px.y / (float)P.ncellsize), cf = floorf(px.x / (float)P.ncellsize);
            bool inside = fabsf(rf) <= 1048576.f && fabsf(cf) <= 1048576.f;      // false for NaN too
            long long idx = 0;
            if (inside) {
                idx = (long long)(int)rf * P.nbwcells + (int)cf;
                inside = idx >= 0 && idx < ncells;
            }
            if (inside) atomicOr(&s_bm[idx >> 5], 1u << (idx & 31));
            else my_oog++;
        }
        double d = -1.;
        const bool skip = (P.filter == OV2_FKF_ONLY_2D && is3d) || (P.filter == OV2_FKF_ONLY_3D && !is3d);
        const int j = skip ? -1 : fkf_find(s_k, n_kf, cur_lmid[g]);
        if (j >= 0) {
            if (P.unrot) d = fkf_unrot_dist(P.K, R, cur_bv + 3 * (size_t)g, kf_unpx[kf0 + j]);
            else d = tri_pdist(cur_unpx[g], kf_unpx[kf0 + j]);
            my_n++;
            const float p = (float)d;
            if (!(fabsf(p) <= 3.402823466e+38f)) my_nf++;
        }
        s_d[i] = d;
    }
    if (my_n) atomicAdd(&s_cnt[0], my_n);
    if (my_nf) atomicAdd(&s_cnt[1], my_nf);
    if (my_3d) atomicAdd(&s_cnt[2], my_3d);
    if (my_oog) atomicAdd(&s_cnt[3], my_oog);
    __syncthreads();                                    // s_d, the bitmap and the counts are complete; the keyframe's ids are done with

    if (count_cells) {
        int c = 0;
        for (int w = t; w < nwords; w += FKF_THREADS) c += __popc(s_bm[w]);
        if (c) atomicAdd(&s_cnt[4], c);
    }
    if (t < 64) {
        // the reference's float sum, in array order: the first wavefront takes 64 distances at a time into registers and every lane
        // adds them one after the other from lane 0 up (a broadcast per term), so the chain of additions never waits for LDS.  A
        // keypoint outside the statistic adds +0: the sum is +0 or above (or NaN) from the start, so that changes no bit of it
        float sum = 0.f;
        for (int base = 0; base < n_cur; base += 64) {
            double d = base + t < n_cur ? s_d[base + t] : -1.;
            if (__ballot(d != -1.) == 0ull) continue;
            if (d == -1.) d = 0.;
            if (P.stat == OV2_FKF_AVG_WIDE) {
                sum = fkf_wide_add64(sum, d);                                                   // :517
            } else {
                const int p = __float_as_int((float)d);
#pragma unroll
                for (int l = 0; l < 64; l++) sum += __int_as_float(__builtin_amdgcn_readlane(p, l));   // :1117-1118
            }
        }
        if (t == 0) s_sum = sum;
    }
    int n_distinct = 0;
    if (P.stat == OV2_FKF_MEDIAN) {                     // std::set<float>: sort, drop repeats, element n_distinct / 2
        int np = FKF_THREADS;
        while (np < n_cur) np <<= 1;
        for (int i = t; i < np; i += FKF_THREADS) {
            int key = FKF_INF_BITS;
            if (i < n_cur) {
                const double d = s_d[i];
                const float p = (float)d;
                if (d != -1. && fabsf(p) <= 3.402823466e+38f) key = __float_as_int(p);
            }
            s_k[i] = key;
        }
        for (int k = 2; k <= np; k <<= 1)
            for (int j = k >> 1; j > 0; j >>= 1) {
                __syncthreads();
                for (int x = t; x < (np >> 1); x += FKF_THREADS) {
                    const int i = ((x & ~(j - 1)) << 1) | (x & (j - 1)), l = i | j;
                    const int a = s_k[i], b = s_k[l];
                    if ((a > b) == ((i & k) == 0)) { s_k[i] = b; s_k[l] = a; }
                }
            }
        __syncthreads();
        const int per = np / FKF_THREADS, first = t * per;
        int c = 0;
        for (int i = first; i < first + per; i++) {
            const int v = s_k[i];
            c += (v != FKF_INF_BITS && (i == 0 || v != s_k[i - 1])) ? 1 : 0;
        }
        const int lane = t & 63, wave = t >> 6;
        int incl = c;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int v = __shfl_up(incl, off, 64);
            if (lane >= off) incl += v;
        }
        if (lane == 63) s_wave[wave] = incl;
        __syncthreads();
        int base = 0;
        for (int w = 0; w < FKF_THREADS / 64; w++) {
            if (w < wave) base += s_wave[w];
            n_distinct += s_wave[w];
        }
        const int excl = base + incl - c, target = n_distinct >> 1;
        if (c > 0 && excl <= target && target < excl + c) {
            int rank = excl;
            for (int i = first; i < first + per; i++) {
                const int v = s_k[i];
                if (v != FKF_INF_BITS && (i == 0 || v != s_k[i - 1])) {
                    if (rank == target) s_med = __int_as_float(v);
                    rank++;
                }
            }
        }
    }
    __syncthreads();
    if (t != 0) return;

    const int n = s_cnt[0], nf = s_cnt[1];
    const float qnan = __int_as_float(0x7fc00000);
    float par;
    if (n == 0) par = P.stat == OV2_FKF_AVG_WIDE ? qnan : 0.f;      // :528 (0.f / 0) / :1126
    else if (P.stat == OV2_FKF_MEDIAN) par = nf > 0 ? qnan : s_med;
    else par = s_sum / (float)n;
    const int nocc = count_cells ? s_cnt[4] : it.noccupcells, nb3d = count_3d ? s_cnt[2] : it.nb3dkps;
    int decision = 0, reason = 0;
    if (P.decide) {                                     // checkNewKfReq, :1005-1045
        const double med = (double)par;
        const int nbimfromkf = it.cur_id - it.kf_id;
        const bool ba = it.localba_is_on != 0;
        if (nf > 0) reason = OV2_KF_NONFINITE;
        else if ((double)nocc < 0.33 * (double)P.nbmaxkps && nbimfromkf >= 5 && !ba) { decision = 1; reason = OV2_KF_RET_FEW_CELLS; }
        else if (nb3d < 20 && nbimfromkf >= 2) { decision = 1; reason = OV2_KF_RET_FEW_3D; }
        else if ((double)nb3d > 0.5 * (double)P.nbmaxkps && (ba || nbimfromkf < 2)) reason = OV2_KF_RET_MANY_3D;
        else if (P.stereo && it.cur_time - it.kf_time > 1. && !ba) { decision = 1; reason = OV2_KF_RET_TIME; }
        else {
            const bool cx = med >= (double)P.finit_parallax / 2. || (P.stereo && !ba && nbimfromkf > 2);
            const bool c0 = med >= (double)P.finit_parallax;
            const bool c1 = (double)nb3d < 0.75 * (double)it.kf_nb3dkps;
            const bool c2 = (double)nocc < 0.5 * (double)P.nbmaxkps && (double)nb3d < 0.85 * (double)it.kf_nb3dkps && !ba;
            decision = ((c0 || c1 || c2) && cx) ? 1 : 0;
            reason = (c0 ? OV2_KF_C0 : 0) | (c1 ? OV2_KF_C1 : 0) | (c2 ? OV2_KF_C2 : 0) | (cx ? OV2_KF_CX : 0);
        }
    }
    int *o = out + FKF_OUT_INTS * (size_t)blockIdx.x;
    o[0] = __float_as_int(par); o[1] = n; o[2] = n_distinct; o[3] = nf;
    o[4] = nocc; o[5] = nb3d; o[6] = s_cnt[3]; o[7] = decision; o[8] = reason;
}

// F: 9 doubles per item.  err / bad: 0 for 3-D keypoints
__global__ __launch_bounds__(FKF_THREADS) void k_fkf_sampson(const FkfItemD *__restrict__ items, const double *__restrict__ F, float thr,
                                                             const int *__restrict__ cur_lmid, const float2 *__restrict__ cur_unpx,
                                                             const uint8_t *__restrict__ cur_is3d, const int *__restrict__ kf_lmid,
                                                             const float2 *__restrict__ kf_unpx, float *__restrict__ err,
                                                             uint8_t *__restrict__ bad)
{
    const FkfItemD &it = items[blockIdx.y];
    const int il = blockIdx.x * FKF_THREADS + threadIdx.x;
    if (il >= it.n_cur) return;
    const int g = it.cur0 + il;
    float e = 0.f;
    if (!cur_is3d[g]) {
        const int j = fkf_find(kf_lmid + it.kf0, it.n_kf, cur_lmid[g]);
        const float2 c = cur_unpx[g];
        const float2 k = j >= 0 ? kf_unpx[it.kf0 + j] : make_float2(0.f, 0.f);     // Keypoint(): unpx_ = (0, 0), :633
        e = sampson(F + 9 * (size_t)blockIdx.y, c.x, c.y, k.x, k.y);               // :639
    }
    err[g] = e;
    bad[g] = e > thr ? 1 : 0;                                                      // :641
}

// k_fkf_parallax as ov2_kf_decision_batch launches it (unrot = 1, OV2_FKF_ALL, OV2_FKF_MEDIAN, decide = 1) on a caller-owned device
// block: the lock-step step (trackb.hip) puts it behind its own kernels.  params must have passed fkf_check_decide.
int ov2_launch_kf_decision(hipStream_t s, const ov2_fkf_params *params, int n_items, const FkfItemD *items_d, const int *cur_lmid,
                           const float2 *cur_px, const float2 *cur_unpx, const double *cur_bv, const uint8_t *cur_is3d, const int *kf_lmid,
                           const float2 *kf_unpx, int *out_d)
{
    FkfParamsD P;
    for (int j = 0; j < 4; j++) P.K[j] = params->K[j];
    P.ncellsize = params->ncellsize; P.nbwcells = params->nbwcells; P.nbhcells = params->nbhcells; P.nbmaxkps = params->nbmaxkps;
    P.finit_parallax = params->finit_parallax; P.stereo = params->stereo ? 1 : 0;
    P.unrot = 1; P.filter = OV2_FKF_ALL; P.stat = OV2_FKF_MEDIAN; P.decide = 1;
    hipLaunchKernelGGL(k_fkf_parallax, dim3(n_items), dim3(FKF_THREADS), 0, s, P, items_d, cur_lmid, cur_px, cur_unpx, cur_bv, cur_is3d,
                       kf_lmid, kf_unpx, out_d);
    OV2_HIP_CHECK(hipGetLastError());
    return OV2_OK;
}

// k_fkf_parallax in the form of ov2_parallax_batch(unrot, filter, stat) on a caller-owned device block: monoinit.hip puts it ahead of
// its own kernels.  cur_unpx is read without unrot, cur_bv with it; the grid fields of params are not read.
int ov2_launch_parallax(hipStream_t s, const ov2_fkf_params *params, int unrot, int filter, int stat, int n_items, const FkfItemD *items_d,
                        const int *cur_lmid, const float2 *cur_unpx, const double *cur_bv, const uint8_t *cur_is3d, const int *kf_lmid,
                        const float2 *kf_unpx, int *out_d)
{
    FkfParamsD P;
    for (int j = 0; j < 4; j++) P.K[j] = params->K[j];
    P.ncellsize = params->ncellsize; P.nbwcells = params->nbwcells; P.nbhcells = params->nbhcells; P.nbmaxkps = params->nbmaxkps;
    P.finit_parallax = params->finit_parallax; P.stereo = params->stereo ? 1 : 0;
    P.unrot = unrot; P.filter = filter; P.stat = stat; P.decide = 0;
    hipLaunchKernelGGL(k_fkf_parallax, dim3(n_items), dim3(FKF_THREADS), 0, s, P, items_d, cur_lmid, (const float2 *)nullptr, cur_unpx,
                       cur_bv, cur_is3d, kf_lmid, kf_unpx, out_d);
    OV2_HIP_CHECK(hipGetLastError());
    return OV2_OK;
}

int fkf_check_decide(const ov2_fkf_params *params)
{
    OV2_REQUIRE(params->ncellsize > 0 && params->nbwcells > 0 && params->nbhcells > 0, OV2_EINVAL,
                "ncellsize / nbwcells / nbhcells not positive");
    OV2_REQUIRE((long long)params->nbwcells * params->nbhcells <= OV2_FKF_MAX_CELLS, OV2_EUNSUPPORTED,
                "more than OV2_FKF_MAX_CELLS (65536) grid cells");
    return OV2_OK;
}

// every input check of the three entry points, before the context is looked at; full: the arrays the parallax / decision kernel reads
int fkf_check_items(int n_items, const ov2_fkf_item *items, bool full, size_t *N, size_t *M, int *n_max)
{
    OV2_REQUIRE(n_items <= 65535, OV2_EUNSUPPORTED, "more than 65535 items in one call");
    *N = *M = 0; *n_max = 0;
    for (int b = 0; b < n_items; b++) {
        const ov2_fkf_item &k = items[b];
        OV2_REQUIRE(k.n_cur >= 0 && k.n_kf >= 0, OV2_EINVAL, "negative count (n_cur / n_kf)");
        OV2_REQUIRE(k.n_cur <= OV2_FKF_MAX_POINTS && k.n_kf <= OV2_FKF_MAX_POINTS, OV2_EUNSUPPORTED,
                    "more than OV2_FKF_MAX_POINTS (2048) keypoints in the frame or the keyframe");
        if (full) OV2_REQUIRE(k.cur_Twc && k.kf_Tcw, OV2_EINVAL, "NULL pose (cur_Twc / kf_Tcw)");
        if (k.n_cur > 0) {
            OV2_REQUIRE(k.cur_lmid && k.cur_unpx && k.cur_is3d, OV2_EINVAL, "NULL array of the current frame (cur_lmid / cur_unpx / cur_is3d)");
            if (full) OV2_REQUIRE(k.cur_px && k.cur_bv, OV2_EINVAL, "NULL array of the current frame (cur_px / cur_bv)");
        }
        if (k.n_kf > 0) {
            OV2_REQUIRE(k.kf_lmid && k.kf_unpx, OV2_EINVAL, "NULL array of the keyframe (kf_lmid / kf_unpx)");
            for (int i = 1; i < k.n_kf; i++) OV2_REQUIRE(k.kf_lmid[i - 1] < k.kf_lmid[i], OV2_EINVAL, "kf_lmid unsorted: not strictly ascending");
        }
        *N += (size_t)k.n_cur; *M += (size_t)k.n_kf;
        *n_max = k.n_cur > *n_max ? k.n_cur : *n_max;
    }
    return OV2_OK;
}

static void fkf_fill_item(FkfItemD &d, const ov2_fkf_item &k, size_t p0, size_t m0, bool full)
{
    memset(&d, 0, sizeof d);
    d.cur0 = (int)p0; d.n_cur = k.n_cur; d.kf0 = (int)m0; d.n_kf = k.n_kf;
    d.cur_id = k.cur_id; d.kf_id = k.kf_id; d.kf_nb3dkps = k.kf_nb3dkps; d.localba_is_on = k.localba_is_on;
    d.noccupcells = k.noccupcells; d.nb3dkps = k.nb3dkps;
    d.cur_time = k.cur_time; d.kf_time = k.kf_time;
    if (full) { memcpy(d.cur_Twc, k.cur_Twc, 56); memcpy(d.kf_Tcw, k.kf_Tcw, 56); }
}

// The item arrays both drivers stage, at their offsets in the host block: the item records, [cur_lmid 4][cur_is3d 1] per current
// keypoint and [kf_lmid 4][kf_unpx 8] per keyframe keypoint always; cur_px, cur_unpx and cur_bv only where the flag says the form
// reads them (their offsets are then not looked at).  !is3d: the flags are zero-filled.  full: the records carry the two poses.
struct FkfIn { size_t o_it, o_lm, o_px, o_un, o_bv, o_3d, o_kl, o_ku; bool full, px, un, bv, is3d; };
static void fkf_stage_items(uint8_t *hs, const FkfIn &s, int n_items, const ov2_fkf_item *items)
{
    size_t p0 = 0, m0 = 0;
    for (int b = 0; b < n_items; b++) {
        const ov2_fkf_item &k = items[b];
        const size_t n = (size_t)k.n_cur, m = (size_t)k.n_kf;
        fkf_fill_item(*(FkfItemD *)(hs + s.o_it + sizeof(FkfItemD) * b), k, p0, m0, s.full);
        if (n) {
            memcpy(hs + s.o_lm + 4 * p0, k.cur_lmid, 4 * n);
            if (s.px) memcpy(hs + s.o_px + 8 * p0, k.cur_px, 8 * n);
            if (s.un) memcpy(hs + s.o_un + 8 * p0, k.cur_unpx, 8 * n);
            if (s.bv) memcpy(hs + s.o_bv + 24 * p0, k.cur_bv, 24 * n);
            if (s.is3d) memcpy(hs + s.o_3d + p0, k.cur_is3d, n); else memset(hs + s.o_3d + p0, 0, n);
        }
        if (m) {
            memcpy(hs + s.o_kl + 4 * m0, k.kf_lmid, 4 * m);
            memcpy(hs + s.o_ku + 8 * m0, k.kf_unpx, 8 * m);
        }
        p0 += n; m0 += m;
    }
}

// results: n_items records of `rec_bytes` (ov2_parallax_result, or ov2_kf_decision_result when decide)
static int fkf_run(ov2_ctx *ctx, const ov2_fkf_params *params, int n_items, const ov2_fkf_item *items, int unrot, int filter, int stat,
                   bool decide, void *results)
{
    OV2_REQUIRE(params, OV2_EINVAL, "NULL params");
    OV2_REQUIRE(n_items >= 0, OV2_EINVAL, "n_items < 0");
    OV2_REQUIRE(n_items == 0 || (items && results), OV2_EINVAL, "NULL item / result array");
    OV2_REQUIRE(unrot == 0 || unrot == 1, OV2_EINVAL, "unrot is not 0 or 1");
    OV2_REQUIRE(filter == OV2_FKF_ALL || filter == OV2_FKF_ONLY_2D || filter == OV2_FKF_ONLY_3D, OV2_EINVAL, "unknown filter");
    OV2_REQUIRE(stat == OV2_FKF_AVG || stat == OV2_FKF_MEDIAN || stat == OV2_FKF_AVG_WIDE, OV2_EINVAL, "unknown stat");
    if (decide) { const int rcd = fkf_check_decide(params);  if (rcd) return rcd; }
    size_t N = 0, M = 0;
    int n_max = 0;
    int rc = fkf_check_items(n_items, items, true, &N, &M, &n_max);
    if (rc) return rc;
    OV2_REQUIRE(ctx, OV2_EINVAL, "NULL context");
    if (n_items == 0) return OV2_OK;
    bool need_px = false, need_3d = filter != OV2_FKF_ALL;
    if (decide)
        for (int b = 0; b < n_items; b++) { need_px |= items[b].noccupcells < 0; need_3d |= items[b].nb3dkps < 0; }
    FkfParamsD P;
    for (int j = 0; j < 4; j++) P.K[j] = params->K[j];
    P.ncellsize = params->ncellsize; P.nbwcells = params->nbwcells; P.nbhcells = params->nbhcells; P.nbmaxkps = params->nbmaxkps;
    P.finit_parallax = params->finit_parallax; P.stereo = params->stereo ? 1 : 0;
    P.unrot = unrot; P.filter = filter; P.stat = stat; P.decide = decide ? 1 : 0;
    // staging: [items 176 B] [cur_lmid 4][cur_px 8][cur_unpx 8][cur_bv 24][cur_is3d 1] per current keypoint, [kf_lmid 4][kf_unpx 8] per
    // keyframe keypoint -- only the arrays this form reads travel (the flags are zero-filled otherwise) --, then FKF_OUT_INTS ints per item
    const size_t B = (size_t)n_items;
    StageCursor c(16);
    const size_t o_it = c.take(sizeof(FkfItemD) * B), o_lm = c.take(4 * N), o_px = c.take(need_px ? 8 * N : 0);
    const size_t o_un = c.take(unrot ? 0 : 8 * N), o_bv = c.take(unrot ? 24 * N : 0), o_3d = c.take(N), o_kl = c.take(4 * M);
    const size_t o_ku = c.take(8 * M), o_out = c.take(4 * FKF_OUT_INTS * B), total = c.off;
    Stage st;
    rc = st.open(ctx, total, total);  if (rc) return rc;
    uint8_t *hs = st.h, *ds = st.d;
    fkf_stage_items(hs, FkfIn{o_it, o_lm, o_px, o_un, o_bv, o_3d, o_kl, o_ku, true, need_px, !unrot, unrot != 0, need_3d}, n_items, items);
    rc = st.upload(0, o_out);  if (rc) return rc;
    hipLaunchKernelGGL(k_fkf_parallax, dim3(n_items), dim3(FKF_THREADS), 0, ctx->stream, P, (const FkfItemD *)(ds + o_it),
                       (const int *)(ds + o_lm), (const float2 *)(ds + o_px), (const float2 *)(ds + o_un), (const double *)(ds + o_bv),
                       (const uint8_t *)(ds + o_3d), (const int *)(ds + o_kl), (const float2 *)(ds + o_ku), (int *)(ds + o_out));
    OV2_HIP_CHECK(hipGetLastError());
    rc = st.download(o_out, total, o_out);  if (rc) return rc;
    rc = st.sync();  if (rc) return rc;
    for (int b = 0; b < n_items; b++) {
        const int *o = (const int *)(hs + o_out) + FKF_OUT_INTS * (size_t)b;
        if (decide) {
            ov2_kf_decision_result &r = ((ov2_kf_decision_result *)results)[b];
            memcpy(&r.parallax, &o[0], 4);
            r.n = o[1]; r.n_distinct = o[2]; r.n_nonfinite = o[3]; r.noccupcells = o[4]; r.nb3dkps = o[5]; r.n_out_of_grid = o[6];
            r.decision = o[7]; r.reason = o[8];
        } else {
            ov2_parallax_result &r = ((ov2_parallax_result *)results)[b];
            memcpy(&r.parallax, &o[0], 4);
            r.n = o[1]; r.n_distinct = o[2]; r.n_nonfinite = o[3];
        }
    }
    return OV2_OK;
}

int ov2_parallax_batch(ov2_ctx *ctx, const ov2_fkf_params *params, int n_items, const ov2_fkf_item *items, int unrot, int filter,
                       int stat, ov2_parallax_result *results)
{
    return fkf_run(ctx, params, n_items, items, unrot, filter, stat, false, results);
}

int ov2_parallax(ov2_ctx *ctx, const ov2_fkf_params *params, const ov2_fkf_item *item, int unrot, int filter, int stat,
                 ov2_parallax_result *result)
{
    OV2_REQUIRE(item && result, OV2_EINVAL, "NULL item / result");
    return fkf_run(ctx, params, 1, item, unrot, filter, stat, false, result);
}

int ov2_kf_decision_batch(ov2_ctx *ctx, const ov2_fkf_params *params, int n_items, const ov2_fkf_item *items,
                          ov2_kf_decision_result *results)
{
    return fkf_run(ctx, params, n_items, items, 1, OV2_FKF_ALL, OV2_FKF_MEDIAN, true, results);
}

int ov2_kf_decision(ov2_ctx *ctx, const ov2_fkf_params *params, const ov2_fkf_item *item, ov2_kf_decision_result *result)
{
    OV2_REQUIRE(item && result, OV2_EINVAL, "NULL item / result");
    return fkf_run(ctx, params, 1, item, 1, OV2_FKF_ALL, OV2_FKF_MEDIAN, true, result);
}

int ov2_sampson_filter_2d_batch(ov2_ctx *ctx, int n_items, const ov2_fkf_item *items, const double *Fkfcur, float fransac_err,
                                ov2_sampson2d_result *results)
{
    OV2_REQUIRE(n_items >= 0, OV2_EINVAL, "n_items < 0");
    OV2_REQUIRE(n_items == 0 || (items && results && Fkfcur), OV2_EINVAL, "NULL item / result array / Fkfcur");
    size_t N = 0, M = 0;
    int n_max = 0;
    int rc = fkf_check_items(n_items, items, false, &N, &M, &n_max);
    if (rc) return rc;
    for (int b = 0; b < n_items; b++)
        OV2_REQUIRE(items[b].n_cur == 0 || (results[b].err && results[b].bad), OV2_EINVAL, "NULL result buffer (err / bad)");
    OV2_REQUIRE(ctx, OV2_EINVAL, "NULL context");
    for (int b = 0; b < n_items; b++) results[b].n_bad = 0;
    if (n_max == 0) return OV2_OK;
    // staging: [items 176 B][F 72 B] [cur_lmid 4][cur_unpx 8][cur_is3d 1] per current keypoint, [kf_lmid 4][kf_unpx 8] per keyframe
    // keypoint, then the outputs [err 4][bad 1] per current keypoint
    const size_t B = (size_t)n_items;
    StageCursor c(16);
    const size_t o_it = c.take(sizeof(FkfItemD) * B), o_f = c.take(72 * B), o_lm = c.take(4 * N), o_un = c.take(8 * N), o_3d = c.take(N);
    const size_t o_kl = c.take(4 * M), o_ku = c.take(8 * M), o_err = c.take(4 * N), o_bad = c.take(N), total = c.off;
    Stage st;
    rc = st.open(ctx, total, total);  if (rc) return rc;
    uint8_t *hs = st.h, *ds = st.d;
    fkf_stage_items(hs, FkfIn{o_it, o_lm, 0, o_un, 0, o_3d, o_kl, o_ku, false, false, true, false, true}, n_items, items);
    memcpy(hs + o_f, Fkfcur, 72 * B);
    rc = st.upload(0, o_err);  if (rc) return rc;
    hipLaunchKernelGGL(k_fkf_sampson, dim3((n_max + FKF_THREADS - 1) / FKF_THREADS, n_items), dim3(FKF_THREADS), 0, ctx->stream,
                       (const FkfItemD *)(ds + o_it), (const double *)(ds + o_f), fransac_err, (const int *)(ds + o_lm),
                       (const float2 *)(ds + o_un), (const uint8_t *)(ds + o_3d), (const int *)(ds + o_kl), (const float2 *)(ds + o_ku),
                       (float *)(ds + o_err), ds + o_bad);
    OV2_HIP_CHECK(hipGetLastError());
    rc = st.download(o_err, total, o_err);  if (rc) return rc;
    rc = st.sync();  if (rc) return rc;
    size_t p0 = 0;
    for (int b = 0; b < n_items; b++) {
        const size_t n = (size_t)items[b].n_cur;
        ov2_sampson2d_result &r = results[b];
        if (!n) continue;
        memcpy(r.err, hs + o_err + 4 * p0, 4 * n);
        memcpy(r.bad, hs + o_bad + p0, n);
        int nb = 0;
        for (size_t i = 0; i < n; i++) nb += r.bad[i] ? 1 : 0;
        r.n_bad = nb;
        p0 += n;
    }
    return OV2_OK;
}

int ov2_sampson_filter_2d(ov2_ctx *ctx, const ov2_fkf_item *item, const double Fkfcur[9], float fransac_err, ov2_sampson2d_result *result)
{
    OV2_REQUIRE(item && result, OV2_EINVAL, "NULL item / result");
    return ov2_sampson_filter_2d_batch(ctx, 1, item, Fkfcur, fransac_err, result);
}
