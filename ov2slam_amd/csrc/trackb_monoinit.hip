// trackb_monoinit.hip -- ov2_btracker_mono_init (f25): trackMono's un-initialised branch on the lock-step tracker's resident state (the
// tracker itself and its steps: trackb.hip, the keyframe calls: trackb_keyframe.hip, the types and helpers they share: trackb.hpp).
// For the items a caller flags, in ONE enqueue and one synchronisation and without a per-slot byte going up: k_minit_input puts the
// resident frame, the resident pose and the resident keyframe's header where the chain of ov2_mono_init reads them (Frame::computeKeypoint
// by k_compute_keypoints, the keyframe's arrays where ov2_btracker_create_keyframe left them), the chain runs on a block of the
// tracker's at capacity (monoinit_dev.hpp), and k_minit_apply puts the result on the resident frame, pose and motion state.  Byte-equal
// to the route of separate calls it replaces (tests/test_gpu_monoinit_lockstep.py).
#include "trackb.hpp"
#include <cmath>

// the block at the rows of this call: the device half grown when the call draws more rows than any before it
static int ensure_minit(ov2_btracker *t, int n_rows, MinitLayout *L)
{
    const char *who = "ov2_btracker_mono_init";
    int rc = minit_layout_capacity(t->batch, t->cfg.n_max, n_rows, L);
    if (rc != OV2_OK) return rc;
    if (n_rows <= t->mi_rows) return OV2_OK;                 // (a layout of fewer rows ends below the one the block was sized for)
    const BtMinitLayout B = bt_minit_layout(t->batch, t->cfg.n_max);
    t->mi_rows = -1;
    const size_t need = B.w_chain + L->total;
    rc = t->mi.h ? t->mi.grow(need, t->ctx->stream, who) : t->mi.alloc(B.i_down, need, t->ctx->stream, who);
    if (rc != OV2_OK) return rc;
    t->mi_rows = n_rows; t->il = B;
    return OV2_OK;
}

extern "C" {

int ov2_btracker_mono_init_begin(ov2_btracker *t, int n_active, const ov2_mono_init_params *params, const uint8_t *do_h,
                                 const unsigned long long *seed_h)
{
    OV2_REQUIRE(t && params && do_h && seed_h, OV2_EINVAL, "ov2_btracker_mono_init: NULL tracker / params / do_h / seed_h");
    OV2_REQUIRE(n_active >= 1 && n_active <= t->batch, OV2_EINVAL, "n_active out of range");
    OV2_REQUIRE(n_active <= 65535, OV2_EINVAL, "more than 65535 items in one call");
    { const int rco = begin_guard(t, CALL_MINIT);  if (rco != OV2_OK) return rco; }
    const ov2_tracker_config &c = t->cfg;
    OV2_REQUIRE(c.n_max >= 1 && c.n_max <= OV2_FKF_MAX_POINTS, OV2_EINVAL,
                "capacity: cfg.n_max outside [1, OV2_FKF_MAX_POINTS (2048)] keypoints of one frame");
    OV2_REQUIRE(t->has_calib, OV2_EINVAL, "ov2_btracker_mono_init: no calibration set on this tracker");
    OV2_REQUIRE(t->fr.d, OV2_EINVAL, "ov2_btracker_mono_init: no resident frame on this tracker (ov2_btracker_set_frame)");
    int rc = minit_check_params(params);  if (rc != OV2_OK) return rc;
    ov2_ctx *ctx = t->ctx;
    OV2_HIP_CHECK(hipSetDevice(ctx->device));
    rc = ensure_epi(t, nullptr);  if (rc != OV2_OK) return rc;
    rc = ensure_mono(t);  if (rc != OV2_OK) return rc;
    MinitLayout M;
    rc = ensure_minit(t, params->n_rows, &M);  if (rc != OV2_OK) return rc;
    ov2_btracker::MinitPending &P = t->ipend;
    P.n_active = n_active;
    P.action.assign((size_t)n_active, OV2_MINIT_NOT_REQUESTED);
    const BtMinitLayout &L = t->il;
    uint8_t *h = t->mi.h, *d = t->mi.d;
    int n_run = 0, n_span = 0;                               // n_span: one past the last item that runs
    for (int b = 0; b < n_active; b++) {
        // :866 pkf == nullptr: no resident keyframe, or none whose info has been set (the rule of ov2_btracker_track_mono)
        const bool no_kf = t->kf_hdr[(size_t)b].n_kf == 0 || !t->res_ki[(size_t)b].has_info;
        const int action = !do_h[b] ? OV2_MINIT_NOT_REQUESTED : (no_kf ? OV2_MINIT_NO_KEYFRAME : OV2_MINIT_READY);   // READY: it runs
        P.action[(size_t)b] = (uint8_t)action;
        h[L.i_act + (size_t)b] = action == OV2_MINIT_READY ? 1 : 0;
        if (action == OV2_MINIT_READY) { n_run++; n_span = b + 1; }
    }
    memcpy(h + L.i_seed, seed_h, 8 * (size_t)n_active);
    t->slot_bytes = 0;
    t->open = CALL_MINIT;
    if (!n_run) return OV2_OK;
    // ---- the one enqueue ----
    const hipStream_t s = ctx->stream;
    const int nm = c.n_max;
    uint8_t *ds = d + L.w_chain;
    MinitTrackArgs a;
    a.f = res_frames(t);
    a.act = d + L.i_act; a.seed = (const unsigned long long *)(d + L.i_seed);
    a.r_T = (double *)(t->res.d + t->nl.r_T); a.r_st = (ov2_motion_state *)(t->res.d + t->nl.r_st); a.hdr = (const FeKfHdr *)t->fx.d;
    a.n_max = nm; a.n_rows = params->n_rows;
    a.nd = (int *)(d + L.w_nd); a.px = (float2 *)(d + L.w_px);
    a.fi = (FkfItemD *)(ds + M.o_fi); a.mi = (MinitItem *)(ds + M.o_mi); a.cur_lmid = (int *)(ds + M.o_lm); a.cur_is3d = ds + M.o_3d;
    a.out = (const MinitOut *)(ds + M.o_out); a.removed = ds + M.o_rm;
    a.rec = (MinitOut *)(d + L.i_rec); a.rm = d + L.i_rm;
    const MinitKf kf{(const int *)(t->depi + t->eL0.o_kl), (const float2 *)(t->depi + t->eL0.o_ku), (const double *)(t->depi + t->eL0.o_kb)};
    // The grids span items [0, n_span): the items behind the last one that runs are never launched; an item inside the span that does
    // not run gets an empty record from k_minit_input (no keypoint, no keyframe), which every kernel of the chain leaves at once.
    rc = [&]() -> int {
        int r = t->mi.up(s, 0, L.i_up);  if (r != OV2_OK) return r;
        r = res_push_sel(t, s);  if (r != OV2_OK) return r;
        r = ov2_launch_minit_input(s, a, n_span);  if (r != OV2_OK) return r;
        r = ov2_launch_compute_keypoints(s, t->calib, (const float *)a.px, nm, a.nd, (float *)(ds + M.o_un), (double *)(ds + M.o_bv), n_span);
        if (r != OV2_OK) return r;
        r = minit_chain_enqueue(s, params, M, ds, n_span, &kf);  if (r != OV2_OK) return r;
        r = ov2_launch_minit_apply(s, a, n_span);  if (r != OV2_OK) return r;
        return t->mi.down(s, L.i_io, L.i_down);
    }();
    if (rc != OV2_OK) {
        // A launch or copy that failed.  Every launch in front of k_minit_apply writes the call's own block only, so the resident
        // state is what it was; if it is the copy behind k_minit_apply that failed, the device has the new pose and motion state and
        // the new frame in the items' OTHER buffers, while res_sel and the host mirrors have not moved: the device then reads the
        // old frame (the buffer res_sel names) with the new pose.  The stream is drained and the error returned; after an OV2_EHIP
        // the caller re-installs the items it flagged (ov2_btracker_set_pose, ov2_btracker_reset_motion) or drops the tracker.
        (void)hipStreamSynchronize(s);
        t->open = CALL_NONE;
    }
    return rc;
}

int ov2_btracker_mono_init_end(ov2_btracker *t, ov2_mono_init_result *results, uint8_t *removed_h)
{
    OV2_REQUIRE(t, OV2_EINVAL, "NULL tracker");
    ov2_btracker::MinitPending &P = t->ipend;
    OV2_REQUIRE(t->open == CALL_MINIT, OV2_EINVAL, "ov2_btracker_mono_init_end without ov2_btracker_mono_init_begin");
    OV2_REQUIRE(results && removed_h, OV2_EINVAL, "ov2_btracker_mono_init_end: NULL result / output array");
    OV2_HIP_CHECK(hipSetDevice(t->ctx->device));
    t->open = CALL_NONE;
    OV2_HIP_CHECK(hipStreamSynchronize(t->ctx->stream));
    const BtMinitLayout &L = t->il;
    const uint8_t *h = t->mi.h;
    const size_t nm = (size_t)t->cfg.n_max;
    for (int b = 0; b < P.n_active; b++) {
        ov2_mono_init_result &r = results[b];
        memset(&r, 0, sizeof r);
        r.action = P.action[(size_t)b];
        r.best_row = -1;
        if (r.action != OV2_MINIT_READY) continue;                       // not requested, or no keyframe: nothing ran for the item
        MinitOut o;
        memcpy(&o, h + L.i_rec + sizeof o * (size_t)b, sizeof o);
        minit_record(o, &r);
        const ResHost src = res_host(t, b, 0);
        const size_t off = nm * (size_t)b, n = (size_t)*src.n;
        const uint8_t *rm = h + L.i_rm + off;
        memcpy(removed_h + off, rm, n);
        r.removed = removed_h + off;
        // the host mirrors, as k_minit_apply left the device
        if (r.action == OV2_MINIT_READY) {
            const ResHost dst = res_host(t, b, 1);
            size_t m = 0;
            for (size_t i = 0; i < n; i++) {
                if (rm[i]) continue;
                dst.px[2 * m] = src.px[2 * i]; dst.px[2 * m + 1] = src.px[2 * i + 1];
                dst.lmid[m] = src.lmid[i];
                dst.is3d[m] = src.is3d[i] ? 1 : 0;
                for (int k = 0; k < 3; k++) dst.wpt[3 * m + k] = src.wpt[3 * i + k];
                m++;
            }
            *dst.n = (int)m;
            t->res_sel[(size_t)b] ^= 1;
            if (m != n) t->res_iskf[(size_t)b] = 0;                      // a slot left: the frame is no longer the keyframe's
            memcpy(t->res_T.data() + 7 * (size_t)b, o.Twc_init, 56);
        }
        ov2_motion_state &st = t->res_st[(size_t)b];                     // MotionModel::reset(): prevTwc_ stays
        st.prev_time = -1.;
        for (int k = 0; k < 6; k++) st.log_relT[k] = 0.;
    }
    return OV2_OK;
}

int ov2_btracker_mono_init(ov2_btracker *t, int n_active, const ov2_mono_init_params *params, const uint8_t *do_h,
                           const unsigned long long *seed_h, ov2_mono_init_result *results, uint8_t *removed_h)
{
    OV2_REQUIRE(results && removed_h, OV2_EINVAL, "ov2_btracker_mono_init: NULL result / output array");
    const int rc = ov2_btracker_mono_init_begin(t, n_active, params, do_h, seed_h);
    if (rc != OV2_OK) return rc;
    return ov2_btracker_mono_init_end(t, results, removed_h);
}

} // extern "C"
