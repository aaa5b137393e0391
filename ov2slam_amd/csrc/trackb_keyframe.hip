// trackb_keyframe.hip -- the lock-step tracker's keyframe calls (ov2_btracker_*; the tracker itself and its steps: trackb.hip, the
// types and helpers both files share: trackb.hpp).
// ov2_btracker_create_keyframe is MapManager::createKeyframe for the items such a step asked to become keyframes (createkf.hip:
// k_ckf_prepare in front, k_ckf_append behind the detector's launches, k_ckf_install behind computeKeypoint and BRIEF): the new frame
// becomes the item's resident keyframe without leaving the device; byte-equal to the separate describe / detect / computeKeypoints
// calls, a host sort and ov2_btracker_set_keyframe + ov2_btracker_set_keyframe_info per item (tests/test_gpu_createkf.py).
// ov2_btracker_stereo_keyframe (stereokf.hip) and ov2_btracker_temporal_keyframe (temporalkf.hip, with the anchor table and its
// setters) triangulate on the resident keyframe; byte-equal to the routes of separate calls they replace (tests/test_gpu_stereokf.py,
// tests/test_gpu_temporalkf.py).
#include "trackb.hpp"
#include <algorithm>
#include <cmath>
#include <vector>

// The resident frame's mirror after a triangulating call on item b, as the call's apply kernel left the device: the other buffer gets
// the frame with the new points (w[i] where st[i] carries `ok`: OV2_TRI_STEREO_OK or OV2_TRI_TEMPORAL_OK) and becomes the current one;
// the keyframe's count of 3-D keypoints
static void res_triangulated(ov2_btracker *t, int b, const uint8_t *st, const double *w, int ok, int nb3dkps)
{
    const ResHost src = res_host(t, b, 0), dst = res_host(t, b, 1);
    const size_t n = (size_t)*src.n;
    memcpy(dst.px, src.px, 8 * n);
    memcpy(dst.lmid, src.lmid, 4 * n);
    for (size_t i = 0; i < n; i++) {
        const bool good = (st[i] & ok) != 0;
        dst.is3d[i] = good || src.is3d[i] ? 1 : 0;
        for (int k = 0; k < 3; k++) dst.wpt[3 * i + k] = good ? w[3 * i + k] : src.wpt[3 * i + k];
    }
    *dst.n = (int)n;
    t->res_sel[(size_t)b] ^= 1;
    t->res_ki[(size_t)b].kf_nb3dkps = nb3dkps;
}

// ---- ov2_btracker_create_keyframe ------------------------------------------------------------------------------------------------
// the detector's work block: every item's output list, then ONE pass's response maps, candidates and free-cell lists (passes of
// `chunk` items follow each other on the context's stream and share them, as the passes of the batched detectors do)
struct CkfWork { int chunk, out_cap; size_t o_out, o_map, o_cand, o_free, total; };
static CkfWork ckf_work(int batch, int cell, int ncells, int mode)
{
    CkfWork W;
    W.chunk = batch < DET_CHUNK / 2 ? batch : DET_CHUNK / 2;
    W.out_cap = det_out_cap(mode, ncells);
    StageCursor c(256);
    W.o_out = c.take(8 * (size_t)W.out_cap * (size_t)batch);
    W.o_map = c.take((size_t)W.chunk * det_map_bytes(cell, ncells, mode));
    W.o_cand = c.take((size_t)W.chunk * (size_t)ncells * DET_CAND_BYTES);
    W.o_free = c.take((size_t)W.chunk * 4 * ((size_t)ncells + 1));
    W.total = c.off;
    return W;
}

// the call's buffers: the I/O block by the first call, the work block grown to `need` bytes
static int ensure_ckf(ov2_btracker *t, size_t need)
{
    const char *who = "ov2_btracker_create_keyframe";
    if (!t->ckf.d) { const int rc = t->ckf.alloc(t->cl.c_down, t->cl.dev_bytes, t->ctx->stream, who);  if (rc) return rc; }
    return need > t->ckw.dev_bytes ? t->ckw.grow(need, t->ctx->stream, who) : OV2_OK;
}

extern "C" {

int ov2_btracker_create_keyframe_begin(ov2_btracker *t, int n_active, const ov2_create_keyframe_params *params,
                                       const ov2_create_keyframe_input *input)
{
    OV2_REQUIRE(t && params && input, OV2_EINVAL, "ov2_btracker_create_keyframe: NULL tracker / params / input");
    const ov2_create_keyframe_params &p = *params;
    const ov2_create_keyframe_input &in = *input;
    const bool resident = !in.px_h;                                      // the frame is the resident one (f21)
    OV2_REQUIRE(resident ? (!in.lmid_h && !in.is3d_h && !in.n_h) : (in.lmid_h && in.is3d_h && in.n_h), OV2_EINVAL,
                "ov2_btracker_create_keyframe: px_h / lmid_h / is3d_h / n_h are all NULL (the resident frame) or none is");
    OV2_REQUIRE(in.make_kf_h && in.nlmid_h && in.nkfid_h && in.time_h, OV2_EINVAL,
                "ov2_btracker_create_keyframe: NULL px_h / lmid_h / is3d_h / n_h / make_kf_h / nlmid_h / nkfid_h / time_h");
    OV2_REQUIRE(p.detector != OV2_CKF_DET_GFTT, OV2_EINVAL, "ov2_btracker_create_keyframe: detectGFTT is not fused (detector OV2_CKF_DET_GFTT)");
    OV2_REQUIRE(p.detector == OV2_CKF_DET_SINGLESCALE || p.detector == OV2_CKF_DET_GRID_FAST, OV2_EINVAL, "ov2_btracker_create_keyframe: unknown detector");
    const int mode = p.detector == OV2_CKF_DET_GRID_FAST ? 0 : 1;
    OV2_REQUIRE(mode == 0 ? in.fast_th_inout != nullptr : in.quality_inout != nullptr, OV2_EINVAL,
                "ov2_btracker_create_keyframe: NULL quality_inout (single scale) / fast_th_inout (grid FAST)");
    OV2_REQUIRE(mode != 0 || p.mask_mode == OV2_MASK_AS_EXECUTED || p.mask_mode == OV2_MASK_INTENDED, OV2_EINVAL, "bad mask_mode");
    OV2_REQUIRE(n_active >= 1 && n_active <= t->batch, OV2_EINVAL, "n_active out of range");
    { const int rco = begin_guard(t, CALL_CKF);  if (rco != OV2_OK) return rco; }
    OV2_REQUIRE(t->raw_which >= 0, OV2_EINVAL, "ov2_btracker_create_keyframe: no current frames (no step yet, or their staging set was uploaded / prepared again)");
    OV2_REQUIRE(n_active <= t->raw_n, OV2_EINVAL, "n_active exceeds the items of the current step");
    OV2_REQUIRE(t->has_calib, OV2_EINVAL, "ov2_btracker_create_keyframe: no calibration set on this tracker");
    OV2_REQUIRE(t->cfg.n_max <= OV2_FKF_MAX_POINTS, OV2_EINVAL, "capacity: cfg.n_max exceeds OV2_FKF_MAX_POINTS (2048) keypoints of one frame");
    OV2_REQUIRE(in.Twc_h || t->res.d, OV2_EINVAL, "ov2_btracker_create_keyframe: Twc_h == NULL on a tracker without a resident pose (ov2_btracker_set_pose / ov2_btracker_track_mono)");
    {
        ov2_fkf_params g;
        memset(&g, 0, sizeof g);
        g.ncellsize = p.ncellsize; g.nbwcells = p.nbwcells; g.nbhcells = p.nbhcells; g.nbmaxkps = p.nbmaxkps;
        const int rcg = fkf_check_decide(&g);  if (rcg != OV2_OK) return rcg;
    }
    const ov2_tracker_config &c = t->cfg;
    OV2_REQUIRE(p.det_cell >= 8, OV2_EINVAL, "the detector's cell size must be at least 8");
    int rc = det_ready(t->ctx, c.w, c.h, p.det_cell, mode);  if (rc != OV2_OK) return rc;
    const int ncells = (c.w / p.det_cell) * (c.h / p.det_cell);
    const size_t nm = (size_t)c.n_max;
    std::vector<int> n_res;                                              // the resident form: the mirror's counts stand for n_h
    if (resident) {
        rc = ensure_res(t);  if (rc != OV2_OK) return rc;
        for (int b = 0; b < n_active; b++) n_res.push_back(*res_host(t, b, 0).n);
    }
    const int *n_h = resident ? n_res.data() : in.n_h;
    bool any = false;
    for (int b = 0; b < n_active; b++) {
        const int n = n_h[b];
        OV2_REQUIRE(n >= 0 && (size_t)n <= nm, OV2_EINVAL, "an item carries more keypoints than cfg.n_max slots");
        if (!in.make_kf_h[b]) continue;
        any = true;
        const int nl = in.nlmid_h[b];
        OV2_REQUIRE(nl >= 0 && (long long)nl + 2ll * ncells <= 2147483647ll, OV2_EINVAL, "nlmid_h negative, or nlmid_h + the detector's capacity overflows int");
        const int *lmid = resident ? res_host(t, b, 0).lmid : in.lmid_h + nm * (size_t)b;
        for (int i = 0; i < n; i++) {
            const int lm = lmid[i];
            OV2_REQUIRE(lm >= 0 && lm < nl, OV2_EINVAL, "lmid_h outside [0, nlmid_h): the map's id counter is monotone");
        }
        OV2_REQUIRE(std::isfinite(in.time_h[b]), OV2_EINVAL, "time not finite");
        const double *T = in.Twc_h ? in.Twc_h + 7 * (size_t)b : t->res_T.data() + 7 * (size_t)b;
        double Ti[7];
        for (int k = 0; k < 7; k++) OV2_REQUIRE(std::isfinite(T[k]), OV2_EINVAL, "pose not finite (Twc_h)");
        ov2_fe_invert(T, Ti);
        for (int k = 0; k < 7; k++) OV2_REQUIRE(std::isfinite(Ti[k]), OV2_EINVAL, "pose not finite (the inverse of Twc_h)");
    }
    ov2_ctx *ctx = t->ctx;
    OV2_HIP_CHECK(hipSetDevice(ctx->device));
    rc = ensure_epi(t, nullptr);  if (rc != OV2_OK) return rc;
    rc = ensure_mono(t);  if (rc != OV2_OK) return rc;
    const bool det_on = ncells > 0;
    const CkfWork W = ckf_work(t->batch, p.det_cell, det_on ? ncells : 1, mode);
    rc = ensure_ckf(t, W.total);  if (rc != OV2_OK) return rc;
    ov2_btracker::CkfPending &P = t->cpend;
    P.n_active = n_active; P.mode = mode; P.ncells = ncells; P.p = p; P.det = det_on && any;
    P.quality = in.quality_inout; P.fast_th = in.fast_th_inout;
    P.flag.assign(in.make_kf_h, in.make_kf_h + n_active);
    P.nkfid.assign(in.nkfid_h, in.nkfid_h + n_active);
    P.time.assign(in.time_h, in.time_h + n_active);
    P.resident = resident;
    P.from_kf = t->from_kf;
    t->slot_bytes = 0;
    // ---- the inputs into the pinned block ----
    const BtCkfLayout &L = t->cl;
    uint8_t *h = t->ckf.h, *d = t->ckf.d;
    const size_t na = (size_t)n_active;
    memcpy(h + L.c_n, n_h, 4 * na);
    for (int b = 0; b < n_active; b++) h[L.c_fl + (size_t)b] = in.make_kf_h[b] ? 1 : 0;
    memcpy(h + L.c_nl, in.nlmid_h, 4 * na);
    memcpy(h + L.c_id, in.nkfid_h, 4 * na);
    memcpy(h + L.c_tm, in.time_h, 8 * na);
    if (in.Twc_h) memcpy(h + L.c_T, in.Twc_h, 56 * na);
    for (int b = 0; b < n_active; b++) {
        if (mode == 0) memcpy(h + L.c_par + 4 * (size_t)b, in.fast_th_inout + b, 4);
        else memcpy(h + L.c_par + 8 * (size_t)b, in.quality_inout + b, 8);
        const size_t n = in.make_kf_h[b] && !resident ? (size_t)in.n_h[b] : 0, o = nm * (size_t)b;
        if (!n) continue;
        memcpy(h + L.c_px + 8 * o, in.px_h + 2 * o, 8 * n);
        memcpy(h + L.c_lm + 4 * o, in.lmid_h + o, 4 * n);
        memcpy(h + L.c_3d + o, in.is3d_h + o, n);
        t->slot_bytes += 13 * n;
    }
    // ---- the one enqueue ----
    const hipStream_t s = ctx->stream;
    const ov2_pyr *pyr = t->pyr[t->cur];
    rc = ov2_pyr_wait_ready(ctx, pyr);  if (rc != OV2_OK) return rc;
    const PyrLevelDesc &L0 = pyr->d.lv[0];
    const uint8_t *im = pyr->d.base + L0.img_roi;
    ResCkfArgs ra;
    if (resident) {
        ra.f = res_frames(t);
        ra.flag = d + L.c_fl; ra.n = (int *)(d + L.c_n); ra.px = (float2 *)(d + L.c_px); ra.lmid = (int *)(d + L.c_lm); ra.is3d = d + L.c_3d;
        ra.rec = (const ov2_create_keyframe_result *)(d + L.c_rec);
    }
    uint8_t *w = t->ckw.d;
    CkfArgs a;
    a.n = (const int *)(d + L.c_n); a.flag = d + L.c_fl; a.nlmid = (const int *)(d + L.c_nl); a.nkfid = (const int *)(d + L.c_id);
    a.time = (const double *)(d + L.c_tm); a.Twc = in.Twc_h ? (const double *)(d + L.c_T) : (const double *)(t->res.d + t->nl.r_T);
    a.px = (float2 *)(d + L.c_px); a.lmid = (int *)(d + L.c_lm); a.is3d = d + L.c_3d;
    a.skip = d + L.w_skip; a.so_n = (const int *)(d + L.c_so); a.so_stride = (int)(sizeof(SelectOut) / sizeof(int));
    a.det = (const float2 *)(w + W.o_out); a.det_cap = W.out_cap; a.nb = (int *)(d + L.w_nb);
    a.img = im; a.img_item = (long long)pyr->d.item_stride; a.img_pitch = L0.img_pitch; a.w = L0.w; a.h = L0.h;
    a.rec = (ov2_create_keyframe_result *)(d + L.c_rec); a.color = d + L.c_col; a.o_hdr = (FeKfHdr *)(d + L.c_hdr); a.perm = (int *)(d + L.c_perm);
    a.unpx = (const float2 *)(d + L.c_un); a.bv = (const double *)(d + L.c_bv);
    a.kf_lmid = (int *)(t->depi + t->eL0.o_kl); a.kf_unpx = (float2 *)(t->depi + t->eL0.o_ku); a.kf_bv = (double *)(t->depi + t->eL0.o_kb);
    a.hdr = (FeKfHdr *)t->fx.d; a.r_ki = (MonoKfInfo *)(t->res.d + t->nl.r_ki); a.r_kt = (double *)(t->res.d + t->nl.r_kt);
    a.n_max = c.n_max; a.ncellsize = p.ncellsize; a.nbwcells = p.nbwcells; a.nbhcells = p.nbhcells; a.nbmaxkps = p.nbmaxkps; a.det_on = det_on ? 1 : 0;
    rc = [&]() -> int {
        // (the resident form: the per-item sections only; k_res_ckf_in fills the per-slot ranges on the device)
        int r = t->ckf.up(s, 0, resident ? L.c_3d : L.c_up);  if (r != OV2_OK) return r;
        if (resident) {
            r = res_push_sel(t, s);  if (r != OV2_OK) return r;
            r = ov2_launch_res_ckf_in(s, ra, n_active);  if (r != OV2_OK) return r;
        }
        r = ov2_launch_ckf_prepare(s, a, n_active);  if (r != OV2_OK) return r;
        if (P.det) {
            // the detectors' three launches per pass, the frame's keypoints as the occupied set, every count left on the device
            for (int c0 = 0; c0 < n_active; c0 += W.chunk) {
                const int n = n_active - c0 < W.chunk ? n_active - c0 : W.chunk;
                DetBatch B = {};
                B.img_stride = (long long)pyr->d.item_stride; B.cur_stride = c.n_max; B.out_stride = W.out_cap;
                B.ncur = a.n + c0; B.skip = a.skip + c0;
                if (mode == 0) B.fast_th = (const int *)(d + L.c_par) + c0; else B.quality = (const double *)(d + L.c_par) + c0;
                r = enqueue_detect(ctx, s, mode, im + (long long)c0 * pyr->d.item_stride, L0.w, L0.h, L0.img_pitch, p.det_cell, n, B, 0, p.mask_mode,
                                    mode == 1 ? p.roi : nullptr, 0.0, 0, (const float2 *)a.px + (size_t)c0 * nm, w + W.o_map, (CellCand *)(w + W.o_cand),
                                    (int *)(w + W.o_free), (float2 *)(w + W.o_out) + (size_t)c0 * (size_t)W.out_cap,
                                    (SelectOut *)(d + L.c_so) + c0, p.do_subpix);
                if (r != OV2_OK) return r;
            }
        }
        r = ov2_launch_ckf_append(s, a, n_active);  if (r != OV2_OK) return r;
        r = ov2_launch_compute_keypoints(s, t->calib, (const float *)a.px, c.n_max, a.nb, (float *)(d + L.c_un), (double *)(d + L.c_bv), n_active);
        if (r != OV2_OK) return r;
        if (p.use_brief) {
            const int which = t->raw_which;
            r = ov2_brief_launch_d(ctx, t->dimg[which], c.w, c.h, t->img_pitch, t->img_bytes, n_active, (const float *)a.px, c.n_max, a.nb, 0,
                                    d + L.c_desc, d + L.c_val);
            if (r != OV2_OK) return r;
            // a later upload of this set on the copy stream orders itself after the reads
            OV2_HIP_CHECK(hipEventRecord(t->used_ev[which], s));
        }
        r = ov2_launch_ckf_install(s, a, n_active);  if (r != OV2_OK) return r;
        if (resident) { r = ov2_launch_res_adopt(s, ra, n_active);  if (r != OV2_OK) return r; }
        if (P.from_kf) {
            // kf_pyr_ = cur_pyr_ (visual_front_end.cpp:52-54) and the keyframe's px_ of every CREATED item, in the same enqueue
            KfPxInstallArgs ka;
            ka.tab = kfpx_table(t);
            ka.make_kf = a.flag; ka.rec = a.rec; ka.px = a.px; ka.lmid = a.lmid; ka.perm = a.perm; ka.adopt = t->kfpx.d + t->kl.k_flag;
            r = ov2_launch_kfpx_install(s, ka, n_active);  if (r != OV2_OK) return r;
            r = ov2_launch_kfpyr_adopt(s, pyr->d, t->kf_store->d, ka.adopt, n_active);  if (r != OV2_OK) return r;
        }
        return t->ckf.down(s, L.c_io, p.use_brief ? L.c_down : L.c_desc);
    }();
    if (rc != OV2_OK) { (void)hipStreamSynchronize(s); return rc; }      // the call stays closed, like its siblings'
    t->open = CALL_CKF;
    return OV2_OK;
}

int ov2_btracker_create_keyframe_end(ov2_btracker *t, ov2_create_keyframe_result *results, float *out_px_h, int *out_lmid_h,
                                     float *unpx_h, double *bv_h, uint8_t *desc_h, uint8_t *valid_h, uint8_t *color_h)
{
    OV2_REQUIRE(t, OV2_EINVAL, "NULL tracker");
    ov2_btracker::CkfPending &P = t->cpend;
    OV2_REQUIRE(t->open == CALL_CKF, OV2_EINVAL, "ov2_btracker_create_keyframe_end without ov2_btracker_create_keyframe_begin");
    OV2_REQUIRE(results && out_px_h && out_lmid_h && unpx_h && bv_h && color_h, OV2_EINVAL, "ov2_btracker_create_keyframe_end: NULL result / output array");
    OV2_REQUIRE(!P.p.use_brief || (desc_h && valid_h), OV2_EINVAL, "ov2_btracker_create_keyframe_end: NULL desc_h / valid_h with use_brief");
    OV2_HIP_CHECK(hipSetDevice(t->ctx->device));
    t->open = CALL_NONE;
    OV2_HIP_CHECK(hipStreamSynchronize(t->ctx->stream));
    const BtCkfLayout &L = t->cl;
    const uint8_t *h = t->ckf.h;
    const size_t nm = (size_t)t->cfg.n_max;
    for (int b = 0; b < P.n_active; b++) {
        if (!P.flag[(size_t)b]) { results[b].action = OV2_CKF_NOT_REQUESTED; continue; }
        ov2_create_keyframe_result &r = results[b];
        memcpy(&r, h + L.c_rec + sizeof r * (size_t)b, sizeof r);
        if (P.det && r.nb2detect > 0) {                                     // the detection ran: the reference's adaptation (:546-552 / :418-423)
            SelectOut so;
            memcpy(&so, h + L.c_so + sizeof so * (size_t)b, sizeof so);
            if (P.mode == 0) P.fast_th[b] = det_adapt_fast_th(P.fast_th[b], so.nbkps, so.nbempty);
            else P.quality[b] = det_adapt_quality(P.quality[b], so.n, P.ncells, so.nboccup);
        }
        if (r.action != OV2_CKF_CREATED) continue;
        const size_t o = nm * (size_t)b, n = (size_t)r.n_kf, n0 = (size_t)r.n_prev;
        memcpy(out_px_h + 2 * o, h + L.c_px + 8 * o, 8 * n);
        memcpy(out_lmid_h + o, h + L.c_lm + 4 * o, 4 * n);
        memcpy(unpx_h + 2 * o, h + L.c_un + 8 * o, 8 * n);
        memcpy(bv_h + 3 * o, h + L.c_bv + 24 * o, 24 * n);
        memcpy(color_h + o + n0, h + L.c_col + o + n0, n - n0);
        if (P.p.use_brief) {
            memcpy(desc_h + 32 * o, h + L.c_desc + 32 * o, 32 * n);
            memcpy(valid_h + o, h + L.c_val + o, n);
        }
        // the host mirrors, as ov2_btracker_set_keyframe / ov2_btracker_set_keyframe_info leave them
        const int *perm = (const int *)(h + L.c_perm) + o, *lm = (const int *)(h + L.c_lm) + o;
        const float *un = (const float *)(h + L.c_un) + 2 * o;
        const double *bv = (const double *)(h + L.c_bv) + 3 * o;
        const KfHost kf = kf_host_item(t, b);
        for (size_t i = 0; i < n; i++) {
            const size_t sl = (size_t)perm[i];
            kf.lmid[i] = lm[sl];
            kf.unpx[2 * i] = un[2 * sl]; kf.unpx[2 * i + 1] = un[2 * sl + 1];
            kf.bv[3 * i] = bv[3 * sl]; kf.bv[3 * i + 1] = bv[3 * sl + 1]; kf.bv[3 * i + 2] = bv[3 * sl + 2];
        }
        memcpy(&t->kf_hdr[(size_t)b], h + L.c_hdr + sizeof(FeKfHdr) * (size_t)b, sizeof(FeKfHdr));
        t->res_ki[(size_t)b] = MonoKfInfo{P.nkfid[(size_t)b], r.nb3dkps, 1, 0};
        t->res_kt[(size_t)b] = P.time[(size_t)b];
        if (P.from_kf) {                                                     // the px table's mirror, as k_kfpx_install left the device
            uint8_t *tab = t->kfpx.h + (size_t)b * t->kl.k_item;
            int *tl = (int *)(tab + t->kl.k_lm);
            float *tp = (float *)(tab + t->kl.k_px);
            const float *px = (const float *)(h + L.c_px) + 2 * o;
            for (size_t i = 0; i < n; i++) {
                const size_t sl = (size_t)perm[i];
                tl[i] = lm[sl]; tp[2 * i] = px[2 * sl]; tp[2 * i + 1] = px[2 * sl + 1];
            }
            *(int *)tab = (int)n;
            t->kf_has_pyr[(size_t)b] = 1;
        } else if (!t->kf_has_pyr.empty()) t->kf_has_pyr[(size_t)b] = 0;    // a keyframe created with the mode off: the store's is stale
        if (!P.resident) {                                                   // the keyframe is no longer the resident frame, if it was
            if (!t->res_iskf.empty()) t->res_iskf[(size_t)b] = 0;
            continue;
        }
        // the resident frame's mirror, as k_res_adopt left the device: the old slots, then the new points without a 3-D point
        const ResHost src = res_host(t, b, 0), dst = res_host(t, b, 1);
        memcpy(dst.px, h + L.c_px + 8 * o, 8 * n);
        memcpy(dst.lmid, lm, 4 * n);
        memcpy(dst.is3d, src.is3d, n0);
        memcpy(dst.wpt, src.wpt, 24 * n0);
        memset(dst.is3d + n0, 0, n - n0);
        memset(dst.wpt + 3 * n0, 0, 24 * (n - n0));
        *dst.n = (int)n;
        t->res_sel[(size_t)b] ^= 1;
        t->res_iskf[(size_t)b] = 1;                                      // the resident frame IS the resident keyframe
    }
    return OV2_OK;
}

int ov2_btracker_create_keyframe(ov2_btracker *t, int n_active, const ov2_create_keyframe_params *params,
                                 const ov2_create_keyframe_input *input, ov2_create_keyframe_result *results, float *out_px_h,
                                 int *out_lmid_h, float *unpx_h, double *bv_h, uint8_t *desc_h, uint8_t *valid_h, uint8_t *color_h)
{
    OV2_REQUIRE(results && out_px_h && out_lmid_h && unpx_h && bv_h && color_h, OV2_EINVAL, "ov2_btracker_create_keyframe: NULL result / output array");
    OV2_REQUIRE(!params || !params->use_brief || (desc_h && valid_h), OV2_EINVAL, "ov2_btracker_create_keyframe: NULL desc_h / valid_h with use_brief");
    const int rc = ov2_btracker_create_keyframe_begin(t, n_active, params, input);
    if (rc != OV2_OK) return rc;
    return ov2_btracker_create_keyframe_end(t, results, out_px_h, out_lmid_h, unpx_h, bv_h, desc_h, valid_h, color_h);
}

} // extern "C"

// ---- the from-keyframe mode: the keyframe store (kltkf.hip) ---------------------------------------------------------------------
static void kf_store_release(ov2_btracker *t)
{
    for (ov2_pyr *v : t->kf_view) ov2_pyr_destroy(v);
    t->kf_view.clear();
    ov2_pyr_destroy(t->kf_store);
    t->kf_store = nullptr;
    t->kfpx.release();
}

// the store, allocated by the first `on`: all of it or nothing
static int ensure_kf_store(ov2_btracker *t)
{
    if (t->kf_store) return OV2_OK;
    const char *who = "ov2_btracker_set_track_from_keyframe";
    const ov2_tracker_config &c = t->cfg;
    OV2_REQUIRE(c.n_max <= OV2_FKF_MAX_POINTS, OV2_EINVAL, "capacity: cfg.n_max exceeds OV2_FKF_MAX_POINTS (2048) keypoints of one frame");
    OV2_HIP_CHECK(hipSetDevice(t->ctx->device));
    int rc = ov2_pyr_create(t->ctx, c.w, c.h, c.win, c.nklt_pyr_lvl, t->batch, &t->kf_store);
    for (int b = 0; b < t->batch && rc == OV2_OK; b++) {
        ov2_pyr *v = nullptr;
        rc = ov2_pyr_item_view(t->kf_store, b, &v);
        if (rc == OV2_OK) t->kf_view.push_back(v);
    }
    if (rc == OV2_OK) rc = t->kfpx.alloc(t->kl.host_bytes, t->kl.dev_bytes, t->ctx->stream, who);
    if (rc != OV2_OK) {
        (void)hipGetLastError();
        kf_store_release(t);
        return rc;
    }
    OV2_HIP_CHECK(hipStreamSynchronize(t->ctx->stream));                 // the store's zero fill
    t->kf_has_pyr.assign((size_t)t->batch, 0);
    return OV2_OK;
}

extern "C" {

int ov2_btracker_set_track_from_keyframe(ov2_btracker *t, int on)
{
    OV2_REQUIRE(t, OV2_EINVAL, "NULL tracker");
    OV2_REQUIRE(!t->open_call(), OV2_EINVAL, "ov2_btracker_set_track_from_keyframe between steps only: a step or a keyframe call is open");
    if (on) {
        int rc = ensure_epi(t, nullptr);  if (rc != OV2_OK) return rc;       // the resident keyframe's lists: membership
        rc = ensure_kf_store(t);  if (rc != OV2_OK) return rc;
    }
    t->from_kf = on != 0;
    return OV2_OK;
}

int ov2_btracker_adopt_keyframe_pyramid(ov2_btracker *t, int n_active, const uint8_t *do_h)
{
    OV2_REQUIRE(t && do_h, OV2_EINVAL, "ov2_btracker_adopt_keyframe_pyramid: NULL tracker / do_h");
    OV2_REQUIRE(!t->open_call(), OV2_EINVAL, "ov2_btracker_adopt_keyframe_pyramid between steps only: a step or a keyframe call is open");
    OV2_REQUIRE(t->kf_store, OV2_EINVAL, "ov2_btracker_adopt_keyframe_pyramid: no keyframe store (ov2_btracker_set_track_from_keyframe)");
    OV2_REQUIRE(n_active >= 1 && n_active <= t->batch, OV2_EINVAL, "n_active out of range");
    OV2_REQUIRE(t->frames > 0, OV2_EINVAL, "ov2_btracker_adopt_keyframe_pyramid: no current frames (no step yet)");
    OV2_HIP_CHECK(hipSetDevice(t->ctx->device));
    const hipStream_t s = t->ctx->stream;
    const ov2_pyr *pyr = t->pyr[t->cur];
    int rc = ov2_pyr_wait_ready(t->ctx, pyr);  if (rc != OV2_OK) return rc;
    const size_t o = t->kl.k_flag;
    for (int b = 0; b < n_active; b++) t->kfpx.h[o + (size_t)b] = do_h[b] ? 1 : 0;
    rc = t->kfpx.up(s, o, o + (size_t)n_active);  if (rc != OV2_OK) return rc;
    rc = ov2_launch_kfpyr_adopt(s, pyr->d, t->kf_store->d, t->kfpx.d + o, n_active);  if (rc != OV2_OK) return rc;
    OV2_HIP_CHECK(hipStreamSynchronize(s));
    for (int b = 0; b < n_active; b++) if (do_h[b]) t->kf_has_pyr[(size_t)b] = 1;
    return OV2_OK;
}

int ov2_btracker_set_keyframe_px(ov2_btracker *t, int item, int n, const int *lmid, const float *px)
{
    OV2_REQUIRE(t, OV2_EINVAL, "NULL tracker");
    OV2_REQUIRE(item >= 0 && item < t->batch, OV2_EINVAL, "batch item out of range");
    OV2_REQUIRE(n >= 0 && n <= t->cfg.n_max, OV2_EINVAL, "ov2_btracker_set_keyframe_px: n outside [0, cfg.n_max]");
    OV2_REQUIRE(n == 0 || (lmid && px), OV2_EINVAL, "ov2_btracker_set_keyframe_px: NULL array");
    for (int i = 0; i < n; i++) {
        OV2_REQUIRE(i == 0 || lmid[i - 1] < lmid[i], OV2_EINVAL, "ov2_btracker_set_keyframe_px: lmid unsorted or repeated: not strictly ascending");
        OV2_REQUIRE(std::isfinite(px[2 * i]) && std::isfinite(px[2 * i + 1]), OV2_EINVAL, "ov2_btracker_set_keyframe_px: px not finite");
    }
    OV2_REQUIRE(!t->open_call(), OV2_EINVAL, "ov2_btracker_set_keyframe_px between steps only: a step or a keyframe call is open");
    OV2_REQUIRE(t->kf_store, OV2_EINVAL, "ov2_btracker_set_keyframe_px: no keyframe store (ov2_btracker_set_track_from_keyframe)");
    OV2_HIP_CHECK(hipSetDevice(t->ctx->device));
    const BtKfPxLayout &K = t->kl;
    const size_t o = (size_t)item * K.k_item;
    uint8_t *tab = t->kfpx.h + o;
    *(int *)tab = n;
    if (n) { memcpy(tab + K.k_lm, lmid, 4 * (size_t)n); memcpy(tab + K.k_px, px, 8 * (size_t)n); }
    const int rc = t->kfpx.up(t->ctx->stream, o, o + K.k_item);  if (rc != OV2_OK) return rc;
    OV2_HIP_CHECK(hipStreamSynchronize(t->ctx->stream));
    return OV2_OK;
}

int ov2_btracker_get_keyframe_px(ov2_btracker *t, int item, int from_device, int *n, int *lmid, float *px)
{
    OV2_REQUIRE(t, OV2_EINVAL, "NULL tracker");
    OV2_REQUIRE(item >= 0 && item < t->batch, OV2_EINVAL, "batch item out of range");
    OV2_REQUIRE(!t->open_call(), OV2_EINVAL, "ov2_btracker_get_keyframe_px between steps only: a step or a keyframe call is open");
    OV2_REQUIRE(t->kf_store, OV2_EINVAL, "ov2_btracker_get_keyframe_px: no keyframe store (ov2_btracker_set_track_from_keyframe)");
    const BtKfPxLayout &K = t->kl;
    const size_t o = (size_t)item * K.k_item;
    const uint8_t *p = t->kfpx.h + o;
    std::vector<uint8_t> dev;
    if (from_device) {
        OV2_HIP_CHECK(hipSetDevice(t->ctx->device));
        dev.resize(K.k_item);
        OV2_HIP_CHECK(hipMemcpyAsync(dev.data(), t->kfpx.d + o, K.k_item, hipMemcpyDeviceToHost, t->ctx->stream));
        OV2_HIP_CHECK(hipStreamSynchronize(t->ctx->stream));
        p = dev.data();
    }
    int m;
    memcpy(&m, p, 4);
    m = m < 0 ? 0 : (m > t->cfg.n_max ? t->cfg.n_max : m);
    if (n) *n = m;
    if (lmid) memcpy(lmid, p + K.k_lm, 4 * (size_t)m);
    if (px) memcpy(px, p + K.k_px, 8 * (size_t)m);
    return OV2_OK;
}

const ov2_pyr *ov2_btracker_kf_item(const ov2_btracker *t, int item)
{
    return t && t->kf_store && item >= 0 && item < t->batch ? t->kf_view[(size_t)item] : nullptr;
}

} // extern "C"

// ---- ov2_btracker_stereo_keyframe (f22) --------------------------------------------------------------------------------------------
// the call's buffers: the pinned block by the first call, the device block regrown when the grid has more cells than any before
static int ensure_skf(ov2_btracker *t, int cells)
{
    const char *who = "ov2_btracker_stereo_keyframe";
    if (cells <= t->skf_cells) return OV2_OK;
    // (the pinned half [0, s_down) does not depend on the cells: it stays when the device half is regrown with the new layout)
    const BtSkfLayout L = bt_skf_layout(t->batch, t->cfg.n_max, cells);
    t->skf_cells = -1;
    const int rc = t->skf.h ? t->skf.grow(L.dev_bytes, t->ctx->stream, who) : t->skf.alloc(L.s_down, L.dev_bytes, t->ctx->stream, who);
    if (rc) return rc;
    t->skf_cells = cells; t->sl = L;
    return OV2_OK;
}

extern "C" {

int ov2_btracker_stereo_keyframe_begin(ov2_btracker *t, int n_active, const ov2_stereo_keyframe_params *params,
                                       const ov2_pyr *right, const uint8_t *do_h)
{
    OV2_REQUIRE(t && params && right && do_h, OV2_EINVAL, "ov2_btracker_stereo_keyframe: NULL tracker / params / right / do_h");
    const ov2_stereo_keyframe_params &p = *params;
    OV2_REQUIRE(n_active >= 1 && n_active <= t->batch, OV2_EINVAL, "n_active out of range");
    OV2_REQUIRE(n_active <= 65535, OV2_EUNSUPPORTED, "more than 65535 items in one call");
    { const int rco = begin_guard(t, CALL_SKF);  if (rco != OV2_OK) return rco; }
    OV2_REQUIRE(t->has_calib, OV2_EINVAL, "ov2_btracker_stereo_keyframe: no calibration set on this tracker");
    OV2_REQUIRE(t->fr.d, OV2_EINVAL, "ov2_btracker_stereo_keyframe: no resident frame on this tracker (ov2_btracker_set_frame)");
    OV2_REQUIRE(t->frames > 0, OV2_EINVAL, "ov2_btracker_stereo_keyframe: no current frames (no step yet)");
    const ov2_tracker_config &c = t->cfg;
    OV2_REQUIRE(c.n_max <= OV2_FKF_MAX_POINTS, OV2_EINVAL, "capacity: cfg.n_max exceeds OV2_FKF_MAX_POINTS (2048) keypoints of one frame");
    const ov2_pyr *left = t->pyr[t->cur];
    {
        const PyrDesc &A = left->d, &R = right->d;
        bool same = R.n_levels == A.n_levels && R.win == A.win;
        for (int l = 0; same && l < A.n_levels; l++) same = R.lv[l].w == A.lv[l].w && R.lv[l].h == A.lv[l].h;
        OV2_REQUIRE(R.batch >= n_active, OV2_EINVAL, "ov2_btracker_stereo_keyframe: the right pyramid has fewer items than n_active");
        OV2_REQUIRE(same, OV2_EINVAL, "ov2_btracker_stereo_keyframe: the right pyramid differs from the tracker's in size, window or level count");
        OV2_REQUIRE(p.nklt_win_size == A.win, OV2_EINVAL, "ov2_btracker_stereo_keyframe: nklt_win_size is not the pyramids' window");
        const int w = p.nklt_win_size;
        OV2_REQUIRE(w == 5 || w == 7 || w == 9 || w == 11 || w == 13, OV2_EUNSUPPORTED, "LK window has no kernel instance (supported: 5,7,9,11,13; the reference ships 9)");
    }
    // the right camera, as ov2_stereo_priors checks it
    OV2_REQUIRE(p.model == OV2_CAM_PINHOLE || p.model == OV2_CAM_FISHEYE, OV2_EINVAL, "unknown camera model");
    OV2_REQUIRE(p.nD >= 0 && (p.nD == 0 || p.D), OV2_EINVAL, "bad distortion vector: nD < 0 or D == NULL");
    OV2_REQUIRE(p.nD == 0 || (p.model == OV2_CAM_FISHEYE ? p.nD == 4 : (p.nD == 4 || p.nD == 5 || p.nD == 8 || p.nD == 12)), OV2_EUNSUPPORTED,
                "unsupported coefficient count: pinhole takes 0 / 4 / 5 / 8 / 12 distortion coefficients, fisheye 0 / 4");
    OV2_REQUIRE(p.img_w > 0 && p.img_h > 0, OV2_EINVAL, "img_w / img_h not positive");     // false for NaN too
    OV2_REQUIRE(p.img_w <= 65536 && p.img_h <= 65536, OV2_EINVAL, "img_w / img_h above 65536");
    const bool rect = p.rect != 0;
    int nbw = 0, nbh = 0;
    if (!rect) {
        OV2_REQUIRE(p.ncellsize > 0, OV2_EINVAL, "ncellsize not positive");
        nbw = (int)ceilf((float)p.img_w / (float)p.ncellsize);              // Frame's grid (frame.cpp:41-43)
        nbh = (int)ceilf((float)p.img_h / (float)p.ncellsize);
        OV2_REQUIRE((long long)nbw * nbh <= OV2_FKF_MAX_CELLS, OV2_EINVAL, "the keypoint grid has more than OV2_FKF_MAX_CELLS (65536) cells");
    }
    const int ncells = nbw * nbh;
    OV2_REQUIRE(p.tri.stereo != 0, OV2_EINVAL, "ov2_btracker_stereo_keyframe: params->tri.stereo == 0 (triangulateStereo runs in stereo mode only)");
    for (int k = 0; k < 7; k++)
        OV2_REQUIRE(std::isfinite(p.Tcic0[k]) && std::isfinite(p.tri.Tcic0[k]) && std::isfinite(p.tri.Tlr[k]), OV2_EINVAL, "pose not finite (Tcic0 / tri.Tcic0 / tri.Tlr)");
    OV2_REQUIRE((size_t)t->batch * (size_t)c.n_max <= 0x7fffffff && (size_t)t->batch * ((size_t)ncells + 1) <= 0x7fffffff, OV2_EUNSUPPORTED,
                "more than 2^31 - 1 elements of one kind in one call");
    KpCalib cr;
    int rc = ov2_kp_calib(p.model, p.K, p.D, p.nD, p.iK, cr);  if (rc != OV2_OK) return rc;
    ov2_ctx *ctx = t->ctx;
    OV2_HIP_CHECK(hipSetDevice(ctx->device));
    rc = ensure_epi(t, nullptr);  if (rc != OV2_OK) return rc;
    rc = ensure_mono(t);  if (rc != OV2_OK) return rc;
    rc = ensure_skf(t, ncells);  if (rc != OV2_OK) return rc;
    ov2_btracker::SkfPending &P = t->spend;
    P.n_active = n_active;
    P.action.assign((size_t)n_active, OV2_SKF_NOT_REQUESTED);
    const BtSkfLayout &L = t->sl;
    uint8_t *h = t->skf.h, *d = t->skf.d;
    int n_done = 0;
    size_t total = 0;
    for (int b = 0; b < n_active; b++) {
        const int action = !do_h[b] ? OV2_SKF_NOT_REQUESTED : (t->res_iskf[(size_t)b] ? OV2_SKF_DONE : OV2_SKF_NOT_KEYFRAME);
        P.action[(size_t)b] = (uint8_t)action;
        h[L.s_act + (size_t)b] = action == OV2_SKF_DONE ? 1 : 0;
        if (action != OV2_SKF_DONE) continue;
        n_done++;
        total += (size_t)*res_host(t, b, 0).n;
    }
    t->slot_bytes = 0;
    t->open = CALL_SKF;
    if (!n_done) return OV2_OK;
    // ---- the one enqueue ----
    const hipStream_t s = ctx->stream;
    rc = ov2_pyr_wait_ready(ctx, left);  if (rc != OV2_OK) { t->open = CALL_NONE; return rc; }
    rc = ov2_pyr_wait_ready(ctx, right);  if (rc != OV2_OK) { t->open = CALL_NONE; return rc; }
    const int lvl = p.nklt_pyr_lvl > left->d.n_levels - 1 ? left->d.n_levels - 1 : (p.nklt_pyr_lvl < 0 ? 0 : p.nklt_pyr_lvl);
    const float up = (float)(1 << lvl), down = 1.f / up;                    // pow(2, nklt_pyr_lvl) and its inverse (:417-418)
    const int nm = c.n_max;
    SkfArgs a;
    a.f = res_frames(t);
    a.act = d + L.s_act; a.hdr = (const FeKfHdr *)t->fx.d; a.r_ki = (MonoKfInfo *)(t->res.d + t->nl.r_ki);
    a.left = t->calib; a.right = cr;
    a.n_max = nm; a.rect = rect ? 1 : 0; a.nbw = nbw; a.nbh = nbh; a.cellsize = (float)p.ncellsize; a.down = down;
    a.pit = (SkfItemD *)(d + L.w_pit); a.tit = (int4 *)(d + L.w_tit); a.Tcw = (double *)(d + L.w_Tcw); a.Twc = (double *)(d + L.w_Twc);
    a.nd = (int *)(d + L.w_nd);
    a.px = (float2 *)(d + L.w_px); a.unpx = (float2 *)(d + L.w_un); a.bv = (double *)(d + L.w_bv); a.fw = (double *)(d + L.w_fw);
    a.top = (float2 *)(d + L.w_top); a.state = d + L.w_st; a.src = (int *)(d + L.w_src);
    a.cell_start = (int *)(d + L.w_cs); a.cell_kp = (int *)(d + L.w_ck);
    a.has_prior = d + L.w_hp; a.flag = d + L.w_fl; a.sadx = (float *)(d + L.w_sx);
    a.lk_out = (const float2 *)(d + L.w_out); a.lk_st = d + L.w_lk; a.gate_ok = d + L.w_ok;
    a.runpx = (float2 *)(d + L.w_ru); a.rbv = (double *)(d + L.w_rbv); a.is_stereo = d + L.w_is;
    a.right_px = (float2 *)(d + L.s_rpx); a.stereo_ok = d + L.s_sok; a.tri_status = d + L.s_tst; a.tri_wpt = (const double *)(d + L.s_wpt);
    a.rec = (ov2_stereo_keyframe_result *)(d + L.s_rec);
    rc = [&]() -> int {
        int r = t->skf.up(s, 0, L.s_up);  if (r != OV2_OK) return r;
        r = res_push_sel(t, s);  if (r != OV2_OK) return r;
        r = ov2_launch_skf_input(s, a, n_active);  if (r != OV2_OK) return r;
        if (total > 0) {
            const int *n_d = a.nd;
            r = ov2_launch_prior_stereo(s, cr, p.Tcic0, p.img_w, p.img_h, p.ncellsize, nbw, nbh, a.rect, a.pit, a.Tcw, (const float *)a.px,
                                        (const float *)a.unpx, a.bv, a.fw, a.state, a.cell_start, a.cell_kp, (float *)(d + L.w_pri), d + L.w_hp,
                                        d + L.w_sk, nm, n_active);
            if (r != OV2_OK) return r;
            r = ov2_launch_skf_seed(s, a, n_active);  if (r != OV2_OK) return r;
            if (rect) {
                r = ov2_launch_line_min_sad(s, left, right, lvl, 7, 1, (const float *)a.top, nm, a.sadx, (float *)(d + L.w_l1), n_d, n_active);
                if (r != OV2_OK) return r;
            }
            r = ov2_launch_track_klt(s, left, right, p.nklt_win_size, 1, lvl, p.max_iter, p.eps, p.nklt_err, p.fmax_fbklt_dist, nm, n_d,
                                     (const float *)a.px, (const float *)(d + L.w_pri), a.flag, (float *)(d + L.w_out), d + L.w_lk, nullptr, a.sadx,
                                     up, ctx->track_impl, n_active, ctx->lk_acc);
            if (r != OV2_OK) return r;
            r = ov2_launch_epipolar_check(s, a.rect, p.Frl, cr, (const float *)a.unpx, (float *)(d + L.w_out), nm, (float *)(d + L.w_gru),
                                          (float *)(d + L.w_err), d + L.w_ok, n_d, n_active);
            if (r != OV2_OK) return r;
            r = ov2_launch_skf_stereo_kp(s, a, n_active);  if (r != OV2_OK) return r;
            r = ov2_launch_triangulate(s, &p.tri, a.tit, a.Twc, nullptr, (const float *)a.unpx, a.bv, (const float *)a.runpx, a.rbv, nullptr, nullptr,
                                       a.src, a.is_stereo, d + L.s_tst, (double *)(d + L.s_wpt), (double *)(d + L.s_inv), nm, n_active);
            if (r != OV2_OK) return r;
        }
        r = ov2_launch_skf_apply(s, a, n_active);  if (r != OV2_OK) return r;
        return t->skf.down(s, L.s_io, L.s_down);
    }();
    if (rc != OV2_OK) { (void)hipStreamSynchronize(s); t->open = CALL_NONE; }      // nothing flips: every frame stays what it was
    return rc;
}

int ov2_btracker_stereo_keyframe_end(ov2_btracker *t, ov2_stereo_keyframe_result *results, float *right_px_h,
                                     uint8_t *stereo_ok_h, uint8_t *tri_status_h, double *wpt_h, double *invdepth_h)
{
    OV2_REQUIRE(t, OV2_EINVAL, "NULL tracker");
    ov2_btracker::SkfPending &P = t->spend;
    OV2_REQUIRE(t->open == CALL_SKF, OV2_EINVAL, "ov2_btracker_stereo_keyframe_end without ov2_btracker_stereo_keyframe_begin");
    OV2_REQUIRE(results && right_px_h && stereo_ok_h && tri_status_h && wpt_h && invdepth_h, OV2_EINVAL,
                "ov2_btracker_stereo_keyframe_end: NULL result / output array");
    OV2_HIP_CHECK(hipSetDevice(t->ctx->device));
    t->open = CALL_NONE;
    OV2_HIP_CHECK(hipStreamSynchronize(t->ctx->stream));
    const BtSkfLayout &L = t->sl;
    const uint8_t *h = t->skf.h;
    const size_t nm = (size_t)t->cfg.n_max;
    for (int b = 0; b < P.n_active; b++) {
        ov2_stereo_keyframe_result &r = results[b];
        memset(&r, 0, sizeof r);
        r.action = P.action[(size_t)b];
        if (r.action != OV2_SKF_DONE) continue;
        memcpy(&r, h + L.s_rec + sizeof r * (size_t)b, sizeof r);
        const size_t o = nm * (size_t)b, n = (size_t)*res_host(t, b, 0).n;
        const uint8_t *st = h + L.s_tst + o;
        const double *w = (const double *)(h + L.s_wpt) + 3 * o;
        memcpy(right_px_h + 2 * o, h + L.s_rpx + 8 * o, 8 * n);
        memcpy(stereo_ok_h + o, h + L.s_sok + o, n);
        memcpy(tri_status_h + o, st, n);
        memcpy(wpt_h + 3 * o, w, 24 * n);
        memcpy(invdepth_h + o, h + L.s_inv + 8 * o, 8 * n);
        // the host mirrors, as k_skf_apply left the device: the frame with the new points, the keyframe's count of 3-D keypoints
        res_triangulated(t, b, st, w, OV2_TRI_STEREO_OK, r.nb3dkps);
    }
    return OV2_OK;
}

int ov2_btracker_stereo_keyframe(ov2_btracker *t, int n_active, const ov2_stereo_keyframe_params *params, const ov2_pyr *right,
                                 const uint8_t *do_h, ov2_stereo_keyframe_result *results, float *right_px_h, uint8_t *stereo_ok_h,
                                 uint8_t *tri_status_h, double *wpt_h, double *invdepth_h)
{
    OV2_REQUIRE(results && right_px_h && stereo_ok_h && tri_status_h && wpt_h && invdepth_h, OV2_EINVAL,
                "ov2_btracker_stereo_keyframe: NULL result / output array");
    const int rc = ov2_btracker_stereo_keyframe_begin(t, n_active, params, right, do_h);
    if (rc != OV2_OK) return rc;
    return ov2_btracker_stereo_keyframe_end(t, results, right_px_h, stereo_ok_h, tri_status_h, wpt_h, invdepth_h);
}

int ov2_btracker_get_keyframe_info(ov2_btracker *t, int item, int from_device, int *kf_id, double *kf_time, int *kf_nb3dkps, int *has_info)
{
    const int rc = mono_item(t, item, "ov2_btracker_get_keyframe_info between steps only: a step is open");
    if (rc != OV2_OK) return rc;
    MonoKfInfo ki = t->res_ki[(size_t)item];
    double kt = t->res_kt[(size_t)item];
    if (from_device) {
        const hipStream_t s = t->ctx->stream;
        OV2_HIP_CHECK(hipMemcpyAsync(&ki, t->res.d + t->nl.r_ki + sizeof ki * (size_t)item, sizeof ki, hipMemcpyDeviceToHost, s));
        OV2_HIP_CHECK(hipMemcpyAsync(&kt, t->res.d + t->nl.r_kt + sizeof kt * (size_t)item, sizeof kt, hipMemcpyDeviceToHost, s));
        OV2_HIP_CHECK(hipStreamSynchronize(s));
    }
    if (kf_id) *kf_id = ki.kf_id;
    if (kf_time) *kf_time = kt;
    if (kf_nb3dkps) *kf_nb3dkps = ki.kf_nb3dkps;
    if (has_info) *has_info = ki.has_info;
    return OV2_OK;
}

} // extern "C"

// ---- ov2_btracker_temporal_keyframe (f23) and the anchor table -----------------------------------------------------------------------
// item b of the anchor mirror: its current table (other == 0) or the buffer its next table is written into (other == 1)
struct AncHost { uint8_t *p; int *n, *lmid, *row; float *unpx; double *bv; int *n_rows, *kfid; double *Twc, *Tcw; };
static AncHost anc_at(const BtTkfLayout &L, uint8_t *p)
{
    return AncHost{p, (int *)(p + L.a_n), (int *)(p + L.a_lm), (int *)(p + L.a_row), (float *)(p + L.a_un), (double *)(p + L.a_bv),
                   (int *)(p + L.a_nr), (int *)(p + L.a_kf), (double *)(p + L.a_Twc), (double *)(p + L.a_Tcw)};
}
static AncHost anc_host(const ov2_btracker *t, int b, int other)
{
    const BtTkfLayout &L = t->tl;
    return anc_at(L, t->anc.h + (size_t)(t->anc_sel[(size_t)b] ^ other) * L.buf_bytes + (size_t)b * L.a_item);
}

static TkfAnchors tkf_anchors(const ov2_btracker *t)
{
    const BtTkfLayout &L = t->tl;
    return TkfAnchors{t->anc.d, L.buf_bytes, L.a_item, L.a_lm, L.a_row, L.a_un, L.a_bv, L.a_nr, L.a_kf, L.a_Twc, L.a_Tcw, t->tkf.d + L.t_sel,
                      t->cfg.n_max, t->n_src_max};
}

// the anchor block, its mirror, the call's blocks and the pose block, allocated by the first call that needs them: every table empty
static int ensure_tkf(ov2_btracker *t, int n_src_max, const char *who)
{
    OV2_REQUIRE(n_src_max >= 1 && n_src_max <= OV2_TKF_MAX_ROWS, OV2_EINVAL, "n_src_max outside [1, OV2_TKF_MAX_ROWS (256)]");
    OV2_REQUIRE(t->cfg.n_max <= OV2_FKF_MAX_POINTS, OV2_EINVAL, "capacity: cfg.n_max exceeds OV2_FKF_MAX_POINTS (2048) keypoints of one frame");
    if (t->anc.d) {
        OV2_REQUIRE(n_src_max == t->n_src_max, OV2_EINVAL, "n_src_max differs from the one this tracker's anchor block was allocated with");
        return OV2_OK;
    }
    OV2_REQUIRE((size_t)t->batch * (size_t)t->cfg.n_max <= 0x7fffffff && (size_t)t->batch * (size_t)n_src_max <= 0x7fffffff, OV2_EUNSUPPORTED,
                "more than 2^31 - 1 elements of one kind in one call");
    OV2_HIP_CHECK(hipSetDevice(t->ctx->device));
    const BtTkfLayout L = bt_tkf_layout(t->batch, t->cfg.n_max, n_src_max);
    const int rc = alloc_all({{&t->anc, L.anchor_bytes, L.anchor_bytes}, {&t->tkf, L.t_down, L.dev_bytes}, {&t->ap, L.pose_bytes, L.pose_bytes}},
                             t->ctx->stream, who);
    if (rc) return rc;
    t->tl = L; t->n_src_max = n_src_max;
    t->anc_sel.assign((size_t)t->batch, 0);
    return OV2_OK;
}

// what the calls around the anchor table share: the item, no open call, the block
static int anc_entry(ov2_btracker *t, int item, const char *open_msg)
{
    OV2_REQUIRE(t, OV2_EINVAL, "NULL tracker");
    OV2_REQUIRE(item >= 0 && item < t->batch, OV2_EINVAL, "batch item out of range");
    OV2_REQUIRE(!t->open_call(), OV2_EINVAL, open_msg);
    OV2_REQUIRE(t->anc.d, OV2_EINVAL, "no anchor block on this tracker (ov2_btracker_reserve_anchors / ov2_btracker_temporal_keyframe)");
    OV2_HIP_CHECK(hipSetDevice(t->ctx->device));
    return OV2_OK;
}

extern "C" {

int ov2_btracker_reserve_anchors(ov2_btracker *t, int n_src_max)
{
    OV2_REQUIRE(t, OV2_EINVAL, "NULL tracker");
    OV2_REQUIRE(!t->open_call(), OV2_EINVAL, "ov2_btracker_reserve_anchors between steps only: a step is open");
    return ensure_tkf(t, n_src_max, "ov2_btracker_reserve_anchors");
}

int ov2_btracker_set_anchors(ov2_btracker *t, int item, int n, const int *lmid, const int *kfid, const float *unpx, const double *bv,
                             int n_rows, const int *row_kfid, const double *row_Twc)
{
    int rc = anc_entry(t, item, "ov2_btracker_set_anchors between steps only: a step is open");
    if (rc != OV2_OK) return rc;
    OV2_REQUIRE(n >= 0 && n <= t->cfg.n_max, OV2_EINVAL, "ov2_btracker_set_anchors: n outside [0, cfg.n_max]");
    OV2_REQUIRE(n_rows >= 0 && n_rows <= t->n_src_max, OV2_EINVAL, "ov2_btracker_set_anchors: n_rows outside [0, n_src_max]");
    OV2_REQUIRE(n == 0 || (lmid && kfid && unpx && bv), OV2_EINVAL, "ov2_btracker_set_anchors: NULL array");
    OV2_REQUIRE(n_rows == 0 || (row_kfid && row_Twc), OV2_EINVAL, "ov2_btracker_set_anchors: NULL array");
    for (int i = 1; i < n; i++) OV2_REQUIRE(lmid[i - 1] < lmid[i], OV2_EINVAL, "ov2_btracker_set_anchors: lmid unsorted: not strictly ascending");
    for (int r = 1; r < n_rows; r++) OV2_REQUIRE(row_kfid[r - 1] < row_kfid[r], OV2_EINVAL, "ov2_btracker_set_anchors: row_kfid unsorted: not strictly ascending");
    std::vector<double> Tcw(7 * (size_t)n_rows);
    for (int r = 0; r < n_rows; r++) {
        for (int c = 0; c < 7; c++) OV2_REQUIRE(std::isfinite(row_Twc[7 * r + c]), OV2_EINVAL, "ov2_btracker_set_anchors: pose not finite (row_Twc)");
        fe_invert_hd(row_Twc + 7 * r, Tcw.data() + 7 * (size_t)r);
        for (int c = 0; c < 7; c++) OV2_REQUIRE(std::isfinite(Tcw[7 * (size_t)r + c]), OV2_EINVAL, "ov2_btracker_set_anchors: pose not finite (the inverse of row_Twc)");
    }
    std::vector<int> row((size_t)n);
    for (int i = 0; i < n; i++) {
        const int *e = std::lower_bound(row_kfid, row_kfid + n_rows, kfid[i]);
        OV2_REQUIRE(e != row_kfid + n_rows && *e == kfid[i], OV2_EINVAL, "ov2_btracker_set_anchors: a kfid that is not among the rows");
        row[(size_t)i] = (int)(e - row_kfid);
        OV2_REQUIRE(std::isfinite(unpx[2 * i]) && std::isfinite(unpx[2 * i + 1]) && std::isfinite(bv[3 * i]) && std::isfinite(bv[3 * i + 1]) &&
                    std::isfinite(bv[3 * i + 2]), OV2_EINVAL, "ov2_btracker_set_anchors: unpx / bv not finite");
    }
    const AncHost a = anc_host(t, item, 0);
    *a.n = n; *a.n_rows = n_rows;
    if (n) { memcpy(a.lmid, lmid, 4 * (size_t)n); memcpy(a.row, row.data(), 4 * (size_t)n); memcpy(a.unpx, unpx, 8 * (size_t)n); memcpy(a.bv, bv, 24 * (size_t)n); }
    if (n_rows) { memcpy(a.kfid, row_kfid, 4 * (size_t)n_rows); memcpy(a.Twc, row_Twc, 56 * (size_t)n_rows); memcpy(a.Tcw, Tcw.data(), 56 * (size_t)n_rows); }
    const hipStream_t s = t->ctx->stream;
    rc = t->anc.up(s, (size_t)(a.p - t->anc.h), (size_t)(a.p - t->anc.h) + t->tl.a_item);  if (rc != OV2_OK) return rc;
    OV2_HIP_CHECK(hipStreamSynchronize(s));
    return OV2_OK;
}

int ov2_btracker_get_anchors(ov2_btracker *t, int item, int from_device, int *n, int *lmid, int *kfid, float *unpx, double *bv,
                             int *n_rows, int *row_kfid, double *row_Twc, double *row_Tcw)
{
    int rc = anc_entry(t, item, "ov2_btracker_get_anchors between steps only: a step is open");
    if (rc != OV2_OK) return rc;
    const BtTkfLayout &L = t->tl;
    AncHost a = anc_host(t, item, 0);
    std::vector<uint8_t> dev;
    if (from_device) {
        dev.resize(L.a_item);
        OV2_HIP_CHECK(hipMemcpyAsync(dev.data(), t->anc.d + (a.p - t->anc.h), L.a_item, hipMemcpyDeviceToHost, t->ctx->stream));
        OV2_HIP_CHECK(hipStreamSynchronize(t->ctx->stream));
        a = anc_at(L, dev.data());
    }
    const int m = std::min(std::max(*a.n, 0), t->cfg.n_max), mr = std::min(std::max(*a.n_rows, 0), t->n_src_max);
    if (n) *n = m;
    if (n_rows) *n_rows = mr;
    if (lmid) memcpy(lmid, a.lmid, 4 * (size_t)m);
    if (unpx) memcpy(unpx, a.unpx, 8 * (size_t)m);
    if (bv) memcpy(bv, a.bv, 24 * (size_t)m);
    if (kfid) for (int i = 0; i < m; i++) kfid[i] = (a.row[i] >= 0 && a.row[i] < mr) ? a.kfid[a.row[i]] : -1;
    if (row_kfid) memcpy(row_kfid, a.kfid, 4 * (size_t)mr);
    if (row_Twc) memcpy(row_Twc, a.Twc, 56 * (size_t)mr);
    if (row_Tcw) memcpy(row_Tcw, a.Tcw, 56 * (size_t)mr);
    return OV2_OK;
}

int ov2_btracker_set_anchor_poses_batch(ov2_btracker *t, int n, const int *item, const int *kfid, const double *Twc, int *n_ignored)
{
    OV2_REQUIRE(t, OV2_EINVAL, "NULL tracker");
    OV2_REQUIRE(!t->open_call(), OV2_EINVAL, "ov2_btracker_set_anchor_poses between steps only: a step is open");
    OV2_REQUIRE(t->anc.d, OV2_EINVAL, "no anchor block on this tracker (ov2_btracker_reserve_anchors / ov2_btracker_temporal_keyframe)");
    OV2_REQUIRE(n >= 0 && (size_t)n <= (size_t)t->batch * (size_t)t->n_src_max, OV2_EINVAL, "ov2_btracker_set_anchor_poses: n outside [0, batch x n_src_max]");
    OV2_REQUIRE(n == 0 || (item && kfid && Twc), OV2_EINVAL, "ov2_btracker_set_anchor_poses: NULL array");
    std::vector<std::pair<int, int>> keys((size_t)n);
    for (int k = 0; k < n; k++) {
        OV2_REQUIRE(item[k] >= 0 && item[k] < t->batch, OV2_EINVAL, "batch item out of range");
        for (int c = 0; c < 7; c++) OV2_REQUIRE(std::isfinite(Twc[7 * (size_t)k + c]), OV2_EINVAL, "ov2_btracker_set_anchor_poses: pose not finite");
        keys[(size_t)k] = std::make_pair(item[k], kfid[k]);
    }
    std::sort(keys.begin(), keys.end());
    for (int k = 1; k < n; k++) OV2_REQUIRE(keys[(size_t)k - 1] != keys[(size_t)k], OV2_EINVAL, "ov2_btracker_set_anchor_poses: the same (item, kfid) twice");
    OV2_HIP_CHECK(hipSetDevice(t->ctx->device));
    // the mirror, and the count of the triples that anchor nothing
    int ignored = 0;
    for (int k = 0; k < n; k++) {
        const AncHost a = anc_host(t, item[k], 0);
        const int mr = std::min(std::max(*a.n_rows, 0), t->n_src_max);
        const int *e = std::lower_bound(a.kfid, a.kfid + mr, kfid[k]);
        if (e == a.kfid + mr || *e != kfid[k]) { ignored++; continue; }
        const size_t r = (size_t)(e - a.kfid);
        memcpy(a.Twc + 7 * r, Twc + 7 * (size_t)k, 56);
        fe_invert_hd(Twc + 7 * (size_t)k, a.Tcw + 7 * r);
    }
    if (n_ignored) *n_ignored = ignored;
    if (n == ignored) return OV2_OK;
    const BtTkfLayout &L = t->tl;
    const hipStream_t s = t->ctx->stream;
    memcpy(t->ap.h + L.p_item, item, 4 * (size_t)n);
    memcpy(t->ap.h + L.p_kfid, kfid, 4 * (size_t)n);
    memcpy(t->ap.h + L.p_Twc, Twc, 56 * (size_t)n);
    memcpy(t->tkf.h + L.t_sel, t->anc_sel.data(), (size_t)t->batch);
    int rc = t->tkf.up(s, L.t_sel, L.t_sel + (size_t)t->batch);  if (rc != OV2_OK) return rc;
    rc = t->ap.up(s, 0, L.p_Twc + 56 * (size_t)n);  if (rc != OV2_OK) return rc;
    rc = ov2_launch_tkf_set_poses(s, tkf_anchors(t), t->batch, n, (const int *)(t->ap.d + L.p_item), (const int *)(t->ap.d + L.p_kfid),
                                            (const double *)(t->ap.d + L.p_Twc));
    OV2_HIP_CHECK(hipStreamSynchronize(s));
    return rc;
}

int ov2_btracker_set_anchor_poses(ov2_btracker *t, int item, int n, const int *kfid, const double *Twc, int *n_ignored)
{
    OV2_REQUIRE(n >= 0 && n <= OV2_TKF_MAX_ROWS, OV2_EINVAL, "ov2_btracker_set_anchor_poses: n outside [0, OV2_TKF_MAX_ROWS]");
    const std::vector<int> items((size_t)n, item);
    return ov2_btracker_set_anchor_poses_batch(t, n, items.data(), kfid, Twc, n_ignored);
}

int ov2_btracker_temporal_keyframe_begin(ov2_btracker *t, int n_active, const ov2_temporal_keyframe_params *params, const uint8_t *do_h)
{
    OV2_REQUIRE(t && params && do_h, OV2_EINVAL, "ov2_btracker_temporal_keyframe: NULL tracker / params / do_h");
    const ov2_temporal_keyframe_params &p = *params;
    OV2_REQUIRE(n_active >= 1 && n_active <= t->batch, OV2_EINVAL, "n_active out of range");
    OV2_REQUIRE(n_active <= 65535, OV2_EUNSUPPORTED, "more than 65535 items in one call");
    { const int rco = begin_guard(t, CALL_TKF);  if (rco != OV2_OK) return rco; }
    OV2_REQUIRE(t->fr.d, OV2_EINVAL, "ov2_btracker_temporal_keyframe: no resident frame on this tracker (ov2_btracker_set_frame)");
    const ov2_tracker_config &c = t->cfg;
    OV2_REQUIRE(c.n_max <= OV2_FKF_MAX_POINTS, OV2_EINVAL, "capacity: cfg.n_max exceeds OV2_FKF_MAX_POINTS (2048) keypoints of one frame");
    for (int k = 0; k < 4; k++) OV2_REQUIRE(std::isfinite(p.tri.K[k]), OV2_EINVAL, "ov2_btracker_temporal_keyframe: params->tri.K not finite");
    for (int k = 0; k < 7; k++)
        OV2_REQUIRE(std::isfinite(p.tri.Tcic0[k]) && std::isfinite(p.tri.Tlr[k]), OV2_EINVAL, "pose not finite (tri.Tcic0 / tri.Tlr)");
    ov2_ctx *ctx = t->ctx;
    OV2_HIP_CHECK(hipSetDevice(ctx->device));
    int rc = ensure_tkf(t, p.n_src_max, "ov2_btracker_temporal_keyframe");  if (rc != OV2_OK) return rc;
    rc = ensure_epi(t, nullptr);  if (rc != OV2_OK) return rc;
    rc = ensure_mono(t);  if (rc != OV2_OK) return rc;
    for (int b = 0; b < n_active; b++) {
        if (!do_h[b] || !t->res_iskf[(size_t)b]) continue;
        const AncHost a = anc_host(t, b, 0);
        const int mr = std::min(std::max(*a.n_rows, 0), t->n_src_max);
        OV2_REQUIRE(mr == 0 || a.kfid[mr - 1] <= t->res_ki[(size_t)b].kf_id, OV2_EINVAL,
                    "ov2_btracker_temporal_keyframe: an item's anchor table holds a keyframe newer than its resident keyframe");
    }
    ov2_btracker::TkfPending &P = t->tpend;
    P.n_active = n_active;
    P.action.assign((size_t)n_active, OV2_TKF_NOT_REQUESTED);
    const BtTkfLayout &L = t->tl;
    uint8_t *h = t->tkf.h, *d = t->tkf.d;
    int n_done = 0;
    for (int b = 0; b < n_active; b++) {
        const int action = !do_h[b] ? OV2_TKF_NOT_REQUESTED : (t->res_iskf[(size_t)b] ? OV2_TKF_DONE : OV2_TKF_NOT_KEYFRAME);
        P.action[(size_t)b] = (uint8_t)action;
        h[L.t_act + (size_t)b] = action == OV2_TKF_DONE ? 1 : 0;
        n_done += action == OV2_TKF_DONE ? 1 : 0;
    }
    memcpy(h + L.t_sel, t->anc_sel.data(), (size_t)t->batch);
    t->slot_bytes = 0;
    t->open = CALL_TKF;
    if (!n_done) return OV2_OK;
    // ---- the one enqueue ----
    const hipStream_t s = ctx->stream;
    const int nm = c.n_max;
    TkfArgs a;
    a.f = res_frames(t);
    a.anc = tkf_anchors(t);
    a.act = d + L.t_act; a.hdr = (FeKfHdr *)t->fx.d; a.r_ki = (MonoKfInfo *)(t->res.d + t->nl.r_ki);
    a.kf_lmid = (int *)(t->depi + t->eL0.o_kl); a.kf_unpx = (float2 *)(t->depi + t->eL0.o_ku); a.kf_bv = (double *)(t->depi + t->eL0.o_kb);
    a.n_max = nm;
    a.tit = (int4 *)(d + L.w_tit); a.Twc = (double *)(d + L.w_Twc); a.ovf = (int *)(d + L.w_ovf); a.srcT = (double *)(d + L.w_srcT);
    a.unpx = (float2 *)(d + L.w_un); a.bv = (double *)(d + L.w_bv); a.src_unpx = (float2 *)(d + L.w_sun); a.src_bv = (double *)(d + L.w_sbv);
    a.src = (int *)(d + L.w_src); a.is_stereo = d + L.w_is;
    a.src_kfid = (int *)(d + L.t_skf); a.tri_status = d + L.t_tst; a.tri_wpt = (const double *)(d + L.t_wpt);
    a.rec = (ov2_temporal_keyframe_result *)(d + L.t_rec);
    rc = [&]() -> int {
        int r = t->tkf.up(s, 0, L.t_up);  if (r != OV2_OK) return r;
        r = res_push_sel(t, s);  if (r != OV2_OK) return r;
        r = ov2_launch_tkf_anchor(s, a, n_active);  if (r != OV2_OK) return r;
        r = ov2_launch_tkf_input(s, a, n_active);  if (r != OV2_OK) return r;
        r = ov2_launch_triangulate(s, &p.tri, a.tit, a.Twc, a.srcT, (const float *)a.unpx, a.bv, nullptr, nullptr, (const float *)a.src_unpx,
                                   a.src_bv, a.src, a.is_stereo, d + L.t_tst, (double *)(d + L.t_wpt), (double *)(d + L.t_inv), nm, n_active);
        if (r != OV2_OK) return r;
        r = ov2_launch_tkf_apply(s, a, n_active);  if (r != OV2_OK) return r;
        return t->tkf.down(s, L.t_io, L.t_down);
    }();
    if (rc != OV2_OK) { (void)hipStreamSynchronize(s); t->open = CALL_NONE; }      // nothing flips: every frame and table stays what it was
    return rc;
}

int ov2_btracker_temporal_keyframe_end(ov2_btracker *t, ov2_temporal_keyframe_result *results, uint8_t *tri_status_h, double *wpt_h,
                                       double *invdepth_h, int *src_kfid_h)
{
    OV2_REQUIRE(t, OV2_EINVAL, "NULL tracker");
    ov2_btracker::TkfPending &P = t->tpend;
    OV2_REQUIRE(t->open == CALL_TKF, OV2_EINVAL, "ov2_btracker_temporal_keyframe_end without ov2_btracker_temporal_keyframe_begin");
    OV2_REQUIRE(results && tri_status_h && wpt_h && invdepth_h && src_kfid_h, OV2_EINVAL,
                "ov2_btracker_temporal_keyframe_end: NULL result / output array");
    OV2_HIP_CHECK(hipSetDevice(t->ctx->device));
    t->open = CALL_NONE;
    OV2_HIP_CHECK(hipStreamSynchronize(t->ctx->stream));
    const BtTkfLayout &L = t->tl;
    const uint8_t *h = t->tkf.h;
    const size_t nm = (size_t)t->cfg.n_max;
    for (int b = 0; b < P.n_active; b++) {
        ov2_temporal_keyframe_result &r = results[b];
        memset(&r, 0, sizeof r);
        r.action = P.action[(size_t)b];
        if (r.action != OV2_TKF_DONE) continue;
        memcpy(&r, h + L.t_rec + sizeof r * (size_t)b, sizeof r);
        if (r.action != OV2_TKF_DONE) continue;                          // OV2_TKF_SRC_OVERFLOW: the device wrote nothing else
        const ResHost src = res_host(t, b, 0);
        const size_t o = nm * (size_t)b, n = (size_t)*src.n;
        const uint8_t *st = h + L.t_tst + o;
        const double *w = (const double *)(h + L.t_wpt) + 3 * o;
        memcpy(tri_status_h + o, st, n);
        memcpy(wpt_h + 3 * o, w, 24 * n);
        memcpy(invdepth_h + o, h + L.t_inv + 8 * o, 8 * n);
        memcpy(src_kfid_h + o, h + L.t_skf + 4 * o, 4 * n);
        // the anchor mirror, by k_tkf_anchor's rule on the keyframe mirror as it was before the call
        const KfHost kf = kf_host_item(t, b);
        int *kl = kf.lmid; float *ku = kf.unpx; double *kb = kf.bv;
        FeKfHdr &hd = t->kf_hdr[(size_t)b];
        const int n_kf = std::min(std::max(hd.n_kf, 0), (int)nm), kfid = t->res_ki[(size_t)b].kf_id;
        {
            const AncHost A = anc_host(t, b, 0), N = anc_host(t, b, 1);
            const int n_o = std::min(std::max(*A.n, 0), (int)nm), n_ro = std::min(std::max(*A.n_rows, 0), t->n_src_max);
            if (n_ro > 0 && A.kfid[n_ro - 1] == kfid) {
                memcpy(N.p, A.p, L.a_item);
            } else {
                std::vector<int> jn((size_t)n_kf, -1), ref((size_t)n_ro, 0), nr((size_t)n_ro, 0);
                for (int i = 0; i < n_kf && n_ro > 0; i++) {
                    const int *e = std::lower_bound(A.lmid, A.lmid + n_o, kl[i]);
                    if (e == A.lmid + n_o || *e != kl[i]) continue;
                    jn[(size_t)i] = (int)(e - A.lmid);
                    ref[(size_t)std::min(std::max(A.row[e - A.lmid], 0), n_ro - 1)] = 1;
                }
                int live = 0;
                for (int q = 0; q < n_ro; q++) { nr[(size_t)q] = live; live += ref[(size_t)q]; }
                for (int i = 0; i < n_kf; i++) {
                    const int j = jn[(size_t)i];
                    N.lmid[i] = kl[i];
                    N.row[i] = j >= 0 ? nr[(size_t)std::min(std::max(A.row[j], 0), n_ro - 1)] : live;
                    memcpy(N.unpx + 2 * i, j >= 0 ? A.unpx + 2 * j : ku + 2 * i, 8);
                    memcpy(N.bv + 3 * i, j >= 0 ? A.bv + 3 * j : kb + 3 * i, 24);
                }
                for (int q = 0; q < n_ro; q++) {
                    if (!ref[(size_t)q]) continue;
                    const int x = nr[(size_t)q];
                    N.kfid[x] = A.kfid[q]; memcpy(N.Twc + 7 * x, A.Twc + 7 * q, 56); memcpy(N.Tcw + 7 * x, A.Tcw + 7 * q, 56);
                }
                N.kfid[live] = kfid; memcpy(N.Twc + 7 * live, hd.kf_Twc, 56); memcpy(N.Tcw + 7 * live, hd.kf_Tcw, 56);
                *N.n = n_kf; *N.n_rows = live + 1;
            }
            t->anc_sel[(size_t)b] ^= 1;
        }
        // the frame's mirror as k_tkf_apply left the device, and the keyframe's without the OV2_TRI_REMOVE_OBS keypoints
        std::vector<int> gone;
        for (size_t i = 0; i < n; i++)
            if (st[i] & OV2_TRI_REMOVE_OBS) gone.push_back(src.lmid[i]);
        res_triangulated(t, b, st, w, OV2_TRI_TEMPORAL_OK, r.nb3dkps);
        if (!gone.empty()) {
            std::sort(gone.begin(), gone.end());
            int m = 0;
            for (int j = 0; j < n_kf; j++) {
                if (std::binary_search(gone.begin(), gone.end(), kl[j])) continue;
                if (m != j) { kl[m] = kl[j]; memcpy(ku + 2 * m, ku + 2 * j, 8); memcpy(kb + 3 * m, kb + 3 * j, 24); }
                m++;
            }
            hd.n_kf = m;
        }
    }
    return OV2_OK;
}

int ov2_btracker_temporal_keyframe(ov2_btracker *t, int n_active, const ov2_temporal_keyframe_params *params, const uint8_t *do_h,
                                   ov2_temporal_keyframe_result *results, uint8_t *tri_status_h, double *wpt_h, double *invdepth_h,
                                   int *src_kfid_h)
{
    OV2_REQUIRE(results && tri_status_h && wpt_h && invdepth_h && src_kfid_h, OV2_EINVAL,
                "ov2_btracker_temporal_keyframe: NULL result / output array");
    const int rc = ov2_btracker_temporal_keyframe_begin(t, n_active, params, do_h);
    if (rc != OV2_OK) return rc;
    return ov2_btracker_temporal_keyframe_end(t, results, tri_status_h, wpt_h, invdepth_h, src_kfid_h);
}

} // extern "C"
