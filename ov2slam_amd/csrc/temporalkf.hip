// temporalkf.hip -- the kernels of ov2_btracker_temporal_keyframe (f23; trackb.hip) around k_triangulate: Mapper::triangulateTemporal
// (src/mapper.cpp:191-343) on the resident keyframe without a map.  What the reference asks its map for -- the first observing keyframe
// of a 2-D keypoint (*co_kf_ids.begin(), :262), that keyframe's keypoint (:292) and its pose (:278, :332) -- is the ANCHOR TABLE of
// the item: one record per keypoint of its latest keyframe, one row per keyframe still referenced.  The item is the grid axis, 256
// threads, no scratch, no atomics.
//   k_tkf_anchor     ONE WORK-GROUP PER ITEM.  The item's next table into its OTHER buffer: a keypoint of the resident keyframe whose
//                    lmid the current table holds (fkf_find) inherits that record, any other anchors at this keyframe with the
//                    kf_unpx / kf_bv k_ckf_install wrote.  The rows some record still refers to are marked in LDS (every lane stores
//                    the same 1) and keep their order; a row's new number is the count of marked rows below it; this keyframe's
//                    row (Twc / Tcw out of the header) goes behind them.  More than n_src_max rows: the overflow flag and nothing
//                    else.  A table whose newest row is this keyframe already is copied as it is.  The rows also go, as (Twc, Tcw)
//                    pairs, where k_triangulate reads its source table.
//   k_tkf_input      one thread per slot of the resident frame: the slot's lmid joined against the resident keyframe (a slot the
//                    keyframe does not hold is no candidate: the reference's getKeypoints2d() of the keyframe) and against the new
//                    table; unpx / bv from the keyframe, src / src_unpx / src_bv from the anchor, src = -1 where the slot is 3-D
//                    (:250) or anchors at this keyframe (:258-266), is_stereo = 0.
//   k_tkf_apply      ONE WORK-GROUP PER ITEM behind k_triangulate: the frame with is3d = 1 and the new point on every
//                    OV2_TRI_TEMPORAL_OK slot into the item's OTHER buffer, the record's counts (a ballot per wavefront, the
//                    wavefronts' sums in LDS), kf_nb3dkps; the OV2_TRI_REMOVE_OBS slots marked on the keyframe in LDS, the keyframe
//                    compacted in order IN PLACE by rounds of 256 keypoints (a round reads before its barrier and writes behind it, to
//                    places below the next round's reads), n_kf lowered in the header.
//   k_tkf_set_poses  one thread per (item, kfid, Twc) triple: the row of that keyframe in the item's current table gets Twc and
//                    Tcw = fe_invert_hd(Twc); a kfid the table does not hold is left alone (the host counts it).
// Every count read from device memory is clamped against n_max / n_src_max before it indexes anything.
#include "temporalkf_dev.hpp"
#include "fkf_dev.hpp"

#pragma clang fp contract(off)

static_assert(sizeof(ov2_temporal_keyframe_result) == 32, "temporal keyframe record");
static_assert(TKF_THREADS == RES_THREADS, "res_rank counts RES_THREADS slots a round");

__device__ __forceinline__ int tkf_min(int a, int b) { return a < b ? a : b; }

__global__ __launch_bounds__(TKF_THREADS) void k_tkf_anchor(TkfArgs a)
{
    __shared__ int s_ref[OV2_TKF_MAX_ROWS];
    const int b = blockIdx.x, t = threadIdx.x;
    if (!a.act[b]) return;
    const int nm = tkf_min(a.n_max, OV2_FKF_MAX_POINTS), ns = tkf_min(a.anc.n_src_max, OV2_TKF_MAX_ROWS);
    const size_t o = (size_t)b * (size_t)a.n_max;
    const TkfItem old = tkf_item(a.anc, b, 0), nw = tkf_item(a.anc, b, 1);
    const int n_kf = res_clamp(a.hdr[b].n_kf, nm), n_o = res_clamp(*old.n, nm), n_ro = res_clamp(*old.n_rows, ns);
    const int kfid = a.r_ki[b].kf_id;
    double *sT = a.srcT + 14 * (size_t)b * (size_t)a.anc.n_src_max;
    if (n_ro > 0 && old.kfid[n_ro - 1] == kfid) {       // (work-group uniform) a second call on this keyframe: the table stays
        for (int i = t; i < n_o; i += TKF_THREADS) {
            nw.lmid[i] = old.lmid[i]; nw.row[i] = old.row[i]; nw.unpx[i] = old.unpx[i];
            nw.bv[3 * i] = old.bv[3 * i]; nw.bv[3 * i + 1] = old.bv[3 * i + 1]; nw.bv[3 * i + 2] = old.bv[3 * i + 2];
        }
        for (int r = t; r < n_ro; r += TKF_THREADS) {
            nw.kfid[r] = old.kfid[r];
#pragma unroll
            for (int c = 0; c < 7; c++) {
                const double w = old.Twc[7 * r + c], v = old.Tcw[7 * r + c];
                nw.Twc[7 * r + c] = w; nw.Tcw[7 * r + c] = v; sT[14 * r + c] = w; sT[14 * r + 7 + c] = v;
            }
        }
        if (t == 0) { *nw.n = n_o; *nw.n_rows = n_ro; a.ovf[b] = 0; }
        return;
    }
    for (int r = t; r < ns; r += TKF_THREADS) s_ref[r] = 0;
    __syncthreads();
    const int *kl = a.kf_lmid + o;
    for (int i = t; i < n_kf; i += TKF_THREADS) {
        const int j = n_ro > 0 ? fkf_find(old.lmid, n_o, kl[i]) : -1;
        if (j >= 0) s_ref[res_clamp(old.row[j], n_ro - 1)] = 1;            // every lane stores the same value
    }
    __syncthreads();
    int n_live = 0;
    for (int r = 0; r < n_ro; r++) n_live += s_ref[r];                     // (every lane reads the same entry: a broadcast)
    if (n_live + 1 > ns) {                                                  // (work-group uniform)
        if (t == 0) a.ovf[b] = 1;
        return;
    }
    for (int i = t; i < n_kf; i += TKF_THREADS) {
        const int lm = kl[i];
        const int j = n_ro > 0 ? fkf_find(old.lmid, n_o, lm) : -1;
        int row = n_live;
        float2 u = a.kf_unpx[o + i];
        double v0 = a.kf_bv[3 * (o + i)], v1 = a.kf_bv[3 * (o + i) + 1], v2 = a.kf_bv[3 * (o + i) + 2];
        if (j >= 0) {
            const int r0 = res_clamp(old.row[j], n_ro - 1);
            row = 0;
            for (int r = 0; r < r0; r++) row += s_ref[r];
            u = old.unpx[j]; v0 = old.bv[3 * j]; v1 = old.bv[3 * j + 1]; v2 = old.bv[3 * j + 2];
        }
        nw.lmid[i] = lm; nw.row[i] = row; nw.unpx[i] = u;
        nw.bv[3 * i] = v0; nw.bv[3 * i + 1] = v1; nw.bv[3 * i + 2] = v2;
    }
    for (int r0 = t; r0 < n_ro; r0 += TKF_THREADS) {
        if (!s_ref[r0]) continue;
        int r = 0;
        for (int q = 0; q < r0; q++) r += s_ref[q];
        nw.kfid[r] = old.kfid[r0];
#pragma unroll
        for (int c = 0; c < 7; c++) {
            const double w = old.Twc[7 * r0 + c], v = old.Tcw[7 * r0 + c];
            nw.Twc[7 * r + c] = w; nw.Tcw[7 * r + c] = v; sT[14 * r + c] = w; sT[14 * r + 7 + c] = v;
        }
    }
    if (t < 7) {
        const double w = a.hdr[b].kf_Twc[t], v = a.hdr[b].kf_Tcw[t];
        nw.Twc[7 * n_live + t] = w; nw.Tcw[7 * n_live + t] = v; sT[14 * n_live + t] = w; sT[14 * n_live + 7 + t] = v;
    }
    if (t == 0) { nw.kfid[n_live] = kfid; *nw.n = n_kf; *nw.n_rows = n_live + 1; a.ovf[b] = 0; }
}

__global__ __launch_bounds__(TKF_THREADS) void k_tkf_input(TkfArgs a)
{
    const int b = blockIdx.y, i = blockIdx.x * TKF_THREADS + threadIdx.x;
    const int nm = tkf_min(a.n_max, OV2_FKF_MAX_POINTS), ns = tkf_min(a.anc.n_src_max, OV2_TKF_MAX_ROWS);
    const size_t o = (size_t)b * (size_t)a.n_max;
    const bool on = a.act[b] != 0 && a.ovf[b] == 0;
    int n = 0;
    ResItem fr = ResItem();
    if (on) { fr = res_item(a.f, b, 0); n = res_clamp(*fr.n, nm); }
    if (i == 0) a.tit[b] = make_int4((int)o, n, b * a.anc.n_src_max, 0);
    if (on && i < 7) a.Twc[7 * (size_t)b + i] = a.hdr[b].kf_Twc[i];
    if (i >= n) return;
    const TkfItem A = tkf_item(a.anc, b, 1);
    const int n_kf = res_clamp(a.hdr[b].n_kf, nm), n_a = res_clamp(*A.n, nm), n_r = res_clamp(*A.n_rows, ns);
    const int kfid = a.r_ki[b].kf_id, lm = fr.lmid[i];
    const int j = fkf_find(a.kf_lmid + o, n_kf, lm);
    const int e = j >= 0 ? fkf_find(A.lmid, n_a, lm) : -1;
    const int row = e >= 0 ? A.row[e] : -1;
    const bool has_row = row >= 0 && row < n_r;
    const int src_kf = has_row ? A.kfid[row] : -1;
    const bool cand = has_row && src_kf != kfid && fr.is3d[i] == 0;        // mapper.cpp:250, :258-266
    const size_t s = o + (size_t)i;
    float2 u = make_float2(0.f, 0.f), su = make_float2(0.f, 0.f);
    double v[3] = {0., 0., 0.}, sv[3] = {0., 0., 0.};
    if (j >= 0) { u = a.kf_unpx[o + j]; v[0] = a.kf_bv[3 * (o + j)]; v[1] = a.kf_bv[3 * (o + j) + 1]; v[2] = a.kf_bv[3 * (o + j) + 2]; }
    if (e >= 0) { su = A.unpx[e]; sv[0] = A.bv[3 * e]; sv[1] = A.bv[3 * e + 1]; sv[2] = A.bv[3 * e + 2]; }
    a.unpx[s] = u; a.bv[3 * s] = v[0]; a.bv[3 * s + 1] = v[1]; a.bv[3 * s + 2] = v[2];
    a.src_unpx[s] = su; a.src_bv[3 * s] = sv[0]; a.src_bv[3 * s + 1] = sv[1]; a.src_bv[3 * s + 2] = sv[2];
    a.src[s] = cand ? row : -1;
    a.is_stereo[s] = 0;
    a.src_kfid[s] = cand ? src_kf : -1;
}

__global__ __launch_bounds__(TKF_THREADS) void k_tkf_apply(TkfArgs a)
{
    __shared__ uint8_t s_rm[OV2_FKF_MAX_POINTS];
    __shared__ int s_tot[TKF_WAVES][5];
    __shared__ int s_w[2][RES_WAVES];
    const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    if (!a.act[b]) return;
    if (a.ovf[b] != 0) {                                                    // (work-group uniform)
        if (t < 8) ((int *)(a.rec + b))[t] = t == 0 ? OV2_TKF_SRC_OVERFLOW : 0;
        return;
    }
    const int nm = tkf_min(a.n_max, OV2_FKF_MAX_POINTS);
    const size_t o = (size_t)b * (size_t)a.n_max;
    const ResItem src = res_item(a.f, b, 0), dst = res_item(a.f, b, 1);
    const int n = res_clamp(*src.n, nm), n_kf = res_clamp(a.hdr[b].n_kf, nm);
    int *kl = a.kf_lmid + o;
    for (int j = t; j < n_kf; j += TKF_THREADS) s_rm[j] = 0;
    __syncthreads();
    int c_tried = 0, c_good = 0, c_rm = 0, c_nomo = 0, c_3d = 0;
    for (int i0 = 0; i0 < n; i0 += TKF_THREADS) {
        const int i = i0 + t;
        const bool in = i < n;
        int st = 0; bool d3 = false;
        if (in) {
            const size_t s = o + (size_t)i;
            st = a.tri_status[s];
            const bool good = (st & OV2_TRI_TEMPORAL_OK) != 0;
            const int lm = src.lmid[i];
            d3 = good || src.is3d[i] != 0;
            dst.px[i] = src.px[i];
            dst.lmid[i] = lm;
            dst.is3d[i] = d3 ? 1 : 0;
            dst.wpt[3 * i] = good ? a.tri_wpt[3 * s] : src.wpt[3 * i];
            dst.wpt[3 * i + 1] = good ? a.tri_wpt[3 * s + 1] : src.wpt[3 * i + 1];
            dst.wpt[3 * i + 2] = good ? a.tri_wpt[3 * s + 2] : src.wpt[3 * i + 2];
            if (st & OV2_TRI_REMOVE_OBS) {                                  // removeMapPointObs(lmid, frame.kfid_): off the KEYFRAME
                const int j = fkf_find(kl, n_kf, lm);
                if (j >= 0) s_rm[j] = 1;                                    // every lane stores the same value
            }
        }
        c_tried += __popcll(__ballot(in && (st & OV2_TRI_TEMPORAL_TRIED) != 0)); c_good += __popcll(__ballot(in && (st & OV2_TRI_TEMPORAL_OK) != 0));
        c_rm += __popcll(__ballot(in && (st & OV2_TRI_REMOVE_OBS) != 0)); c_nomo += __popcll(__ballot(in && (st & OV2_TRI_NO_MOTION) != 0));
        c_3d += __popcll(__ballot(in && d3));
    }
    if (lane == 0) { s_tot[wave][0] = c_tried; s_tot[wave][1] = c_good; s_tot[wave][2] = c_rm; s_tot[wave][3] = c_nomo; s_tot[wave][4] = c_3d; }
    __syncthreads();
    // the keyframe without the marked keypoints, in order, in place: round k reads [256 k, 256 k + 256) in front of res_rank's barrier
    // and writes behind it to places <= the ones it read, all of them below what round k + 1 reads
    int m = 0;
    for (int j0 = 0, round = 0; j0 < n_kf; j0 += TKF_THREADS, round++) {
        const int j = j0 + t;
        const bool keep = j < n_kf && s_rm[j] == 0;
        int lm = 0; float2 u = make_float2(0.f, 0.f); double v0 = 0., v1 = 0., v2 = 0.;
        if (keep) { lm = kl[j]; u = a.kf_unpx[o + j]; v0 = a.kf_bv[3 * (o + j)]; v1 = a.kf_bv[3 * (o + j) + 1]; v2 = a.kf_bv[3 * (o + j) + 2]; }
        const int r = res_rank(keep, round, s_w, m);
        if (keep && r != j) {
            kl[r] = lm; a.kf_unpx[o + r] = u;
            a.kf_bv[3 * (o + r)] = v0; a.kf_bv[3 * (o + r) + 1] = v1; a.kf_bv[3 * (o + r) + 2] = v2;
        }
    }
    if (t != 0) return;
    int v[5] = {0, 0, 0, 0, 0};
#pragma unroll
    for (int w = 0; w < TKF_WAVES; w++)
#pragma unroll
        for (int k = 0; k < 5; k++) v[k] += s_tot[w][k];
    *dst.n = n;
    ov2_temporal_keyframe_result r;
    r.action = OV2_TKF_DONE; r.n = n; r.n_candidates = v[0]; r.n_temporal_good = v[1]; r.n_remove_obs = v[2]; r.n_no_motion = v[3];
    r.nb3dkps = v[4]; r.n_rows = res_clamp(*tkf_item(a.anc, b, 1).n_rows, a.anc.n_src_max);
    a.rec[b] = r;
    a.r_ki[b].kf_nb3dkps = v[4];                                             // updateMapPoint -> turnKeypoint3d on the keyframe
    a.hdr[b].n_kf = m;
}

__global__ __launch_bounds__(TKF_THREADS) void k_tkf_set_poses(TkfAnchors anc, int batch, int n, const int *__restrict__ item,
                                                               const int *__restrict__ kfid, const double *__restrict__ Twc)
{
    const int k = blockIdx.x * TKF_THREADS + threadIdx.x;
    if (k >= n) return;
    const int b = item[k];
    if (b < 0 || b >= batch) return;
    const TkfItem A = tkf_item(anc, b, 0);
    const int n_r = res_clamp(*A.n_rows, tkf_min(anc.n_src_max, OV2_TKF_MAX_ROWS));
    const int r = fkf_find(A.kfid, n_r, kfid[k]);                           // the rows ascend by kfid
    if (r < 0) return;
    double T[7], Ti[7];
#pragma unroll
    for (int c = 0; c < 7; c++) T[c] = Twc[7 * (size_t)k + c];
    fe_invert_hd(T, Ti);
#pragma unroll
    for (int c = 0; c < 7; c++) { A.Twc[7 * r + c] = T[c]; A.Tcw[7 * r + c] = Ti[c]; }
}

int ov2_launch_tkf_anchor(hipStream_t s, const TkfArgs &a, int n_active)
{
    hipLaunchKernelGGL(k_tkf_anchor, dim3(n_active), dim3(TKF_THREADS), 0, s, a);
    OV2_HIP_CHECK(hipGetLastError());
    return OV2_OK;
}

int ov2_launch_tkf_input(hipStream_t s, const TkfArgs &a, int n_active)
{
    hipLaunchKernelGGL(k_tkf_input, dim3((a.n_max + TKF_THREADS - 1) / TKF_THREADS, n_active), dim3(TKF_THREADS), 0, s, a);
    OV2_HIP_CHECK(hipGetLastError());
    return OV2_OK;
}

int ov2_launch_tkf_apply(hipStream_t s, const TkfArgs &a, int n_active)
{
    hipLaunchKernelGGL(k_tkf_apply, dim3(n_active), dim3(TKF_THREADS), 0, s, a);
    OV2_HIP_CHECK(hipGetLastError());
    return OV2_OK;
}

int ov2_launch_tkf_set_poses(hipStream_t s, const TkfAnchors &anc, int batch, int n, const int *item_d, const int *kfid_d, const double *Twc_d)
{
    hipLaunchKernelGGL(k_tkf_set_poses, dim3((n + TKF_THREADS - 1) / TKF_THREADS), dim3(TKF_THREADS), 0, s, anc, batch, n, item_d, kfid_d, Twc_d);
    OV2_HIP_CHECK(hipGetLastError());
    return OV2_OK;
}
