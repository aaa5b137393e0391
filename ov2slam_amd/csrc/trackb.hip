// trackb.hip -- lock-step tracker: `batch` camera streams advance one frame per call (ov2_btracker_*).
//
// The offline / batch mode of the reference's benchmark protocol (/root/reference/benchmark_scripts/euroc_bench.sh:3-27 plays whole
// sequences; BASELINE.json configs[4] shards 11 of them over the GPUs of a node).  A rank that owns several sequences can push
// each through its own ov2_tracker (track.hip) -- every stream is then a chain of ~10 small dependent launches per frame and the
// streams together saturate the command processor's launch rate with the CUs ~5 % busy (profiles/archive/r4_stream_concurrency.txt).
// Here the per-frame enqueue of VisualFrontEnd::preprocessImage + VisualFrontEnd::kltTracking (+ Frame::computeKeypoint)
// (src/visual_front_end.cpp:1143-1177, :132-275; src/frame.cpp:246-254) is issued ONCE for all streams: the same kernels as
// track.hip -- CLAHE, pyramid levels, the fused kltTracking kernel (lkw.hip / lk.hip), k_compute_keypoints -- with the grid
// extended by the batch item.  Per step: one H2D of the frames, the kernels, one synchronisation.  Items [0, n_active) take part
// (sequences of different length drop out from the tail).
// An offline host knows frame f + 1 while frame f is tracked: the step is a three-stage pipeline on three streams --
//   copy stream      H2D of frame f + 2                       (ov2_btracker_upload)
//   prep stream      CLAHE + pyramid of frame f + 1           (ov2_btracker_prepare; into the NEXT pyramid set)
//   context stream   kltTracking + computeKeypoint of frame f (ov2_btracker_track_frame: waits for its pyramids, one sync)
// with three pinned staging sets and eight pyramid sets in rotation; events order producer -> consumer and consumer -> the producer
// that reuses a buffer.  A caller that uses neither look-ahead call gets the same results from the plain in-order enqueue.
// Results per item are bit-identical to an ov2_tracker fed the same frames and keypoints (tests/test_gpu_lockstep.py).
// ov2_btracker_track_frame_pose puts computePose behind the step's kernels on the context's stream (framepose.hip: the pose set and
// P3P's sample table; pose_dev.hpp: the chain of pnp.hip on a block at capacity): tracking results and the per-frame pose with the
// one synchronisation, byte-equal to ov2_btracker_track_frame_map followed by ov2_compute_pose_batch (tests/test_gpu_framepose.py).
// ov2_btracker_track_frame_epi_pose is that step with epipolar2d2dFiltering between the select and the pack (frameepi.hip: the frame
// packed into the epipolar block, the chain of epifilter.hip on it, the removals applied to the select bytes), against a keyframe
// that ov2_btracker_set_keyframe keeps on the device: trackMono's per-frame sequence with doepipolar_ == 1 in one enqueue, byte-equal
// to the three separate calls (tests/test_gpu_frameepi.py).
// ov2_btracker_track_mono is trackMono after initialisation: that step (or the pose step, doepipolar_ == 0) between the motion model
// and the keyframe decision (mono.hip: k_mono_apply in front, k_mono_pack and fkf.hip's k_fkf_parallax behind), the frame pose, the
// motion state and the keyframe's id / time / nb3dkps resident on the device with host mirrors; byte-equal to ov2_motion_apply_batch,
// the step, ov2_motion_update_batch and ov2_kf_decision_batch (tests/test_gpu_trackmono.py).
// The keyframe calls on this state (ov2_btracker_create_keyframe, _stereo_keyframe, _temporal_keyframe and the anchor table) are
// trackb_keyframe.hip; struct ov2_btracker, the block types and the helpers both files use are declared in trackb.hpp.
// The resident frame (ov2_btracker_set_frame / _get_frame / _update_frame, ov2_btracker_track_mono_resident, create_keyframe with
// px_h == NULL; resident.hip): the current frame of every item -- px, lmid, is3d, wpt per slot -- stays on the device between those
// calls, in a block of two buffers per item with a pinned mirror of the same layout.  k_res_stage writes it where the step's kernels
// read their per-slot inputs (which are then not copied up), k_res_carry writes the frame the step leaves by k_mono_pack's rule,
// k_res_update applies what the map did, k_res_ckf_in / k_res_adopt put create_keyframe on it; byte-equal to the same cycle on frames
// kept on the host (tests/test_gpu_resident.py; tests/resident_ref.py is that cycle).
#include "trackb.hpp"
#include <algorithm>
#include <cmath>
#include <new>
#include <vector>

static_assert(sizeof(PoseOut) == BT_POSE_OUT_BYTES, "trackb_layout.hpp: the pose block's record");
static_assert(sizeof(EpifOut) == BT_EPIF_OUT_BYTES, "trackb_layout.hpp: the epipolar block's record");
static_assert(sizeof(FeKfHdr) == BT_KF_HDR_BYTES, "trackb_layout.hpp: the index block's header");
static_assert(sizeof(ov2_motion_state) == BT_MOTION_STATE_BYTES, "trackb_layout.hpp: the mono blocks' state");
static_assert(sizeof(FkfItemD) == BT_FKF_ITEM_BYTES && 4 * FKF_OUT_INTS == BT_KF_DEC_BYTES, "trackb_layout.hpp: the mono blocks' records");
static_assert(sizeof(ov2_create_keyframe_result) == BT_CKF_REC_BYTES && sizeof(SelectOut) == BT_CKF_SO_BYTES, "trackb_layout.hpp: the createKeyframe block's records");
static_assert(sizeof(ov2_stereo_keyframe_result) == BT_SKF_REC_BYTES && sizeof(SkfItemD) == 16, "trackb_layout.hpp: the stereo keyframe block's records");
static_assert(sizeof(ov2_temporal_keyframe_result) == BT_TKF_REC_BYTES, "trackb_layout.hpp: the temporal keyframe block's record");
static_assert(sizeof(MinitOut) == BT_MINIT_REC_BYTES, "trackb_layout.hpp: the mono initialisation block's record");
static_assert(sizeof(ov2_resident_op) == BT_RES_OP_BYTES && sizeof(ov2_resident_update_result) == BT_RES_REC_BYTES, "trackb_layout.hpp: the resident frame's records");

// ---- the block types (trackb.hpp) ----
int IoBlock::alloc(size_t n, bool &zero_copy, bool decide, const char *who)
{
    hipError_t e = hipHostMalloc((void **)&h, n, hipHostMallocMapped);
    void *alias = nullptr;
    if (e == hipSuccess && decide) {
        zero_copy = hipHostGetDevicePointer(&alias, h, 0) == hipSuccess && alias;
        if (!zero_copy) (void)hipGetLastError();
    }
    if (e == hipSuccess && !zero_copy) { e = hipMalloc((void **)&d, n); alias = d; }
    else if (e == hipSuccess && !decide) e = hipHostGetDevicePointer(&alias, h, 0);
    if (e != hipSuccess || !alias) {
        release();
        (void)hipGetLastError();
        ov2_set_error("%s: %s", who, hipGetErrorString(e));
        return OV2_ENOMEM;
    }
    memset(h, 0, n);
    k = (uint8_t *)alias; bytes = n;
    return OV2_OK;
}
void IoBlock::release()
{
    if (h) (void)hipHostFree(h);
    if (d) (void)hipFree(d);
    h = d = k = nullptr; bytes = 0;
}
int IoBlock::upload(hipStream_t s, size_t from, size_t to) const
{
    if (d && to > from) OV2_HIP_CHECK(hipMemcpyAsync(d + from, h + from, to - from, hipMemcpyHostToDevice, s));
    return OV2_OK;
}
int IoBlock::download(hipStream_t s, size_t from, size_t to) const
{
    if (d) OV2_HIP_CHECK(hipMemcpyAsync(h + from, d + from, to - from, hipMemcpyDeviceToHost, s));
    return OV2_OK;
}

int DevBlock::fail(hipError_t e, const char *who)
{
    release();
    (void)hipGetLastError();
    ov2_set_error("%s: %s", who, hipGetErrorString(e));
    return OV2_ENOMEM;
}
int DevBlock::alloc(size_t host_bytes, size_t n, hipStream_t s, const char *who)
{
    release();
    const hipError_t e = host_bytes ? hipHostMalloc((void **)&h, host_bytes, hipHostMallocDefault) : hipSuccess;
    if (e != hipSuccess) return fail(e, who);
    if (h) memset(h, 0, host_bytes);
    return grow(n, s, who);
}
int DevBlock::grow(size_t need, hipStream_t s, const char *who)
{
    OV2_HIP_CHECK(hipStreamSynchronize(s));                              // (an earlier call's kernels have long finished: its _end waited)
    if (d) (void)hipFree(d);
    d = nullptr; dev_bytes = 0;
    hipError_t e = hipMalloc((void **)&d, need);
    if (e == hipSuccess) e = hipMemsetAsync(d, 0, need, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return fail(e, who);
    dev_bytes = need;
    return OV2_OK;
}
void DevBlock::release()
{
    if (h) (void)hipHostFree(h);
    if (d) (void)hipFree(d);
    h = d = nullptr; dev_bytes = 0;
}
int DevBlock::up(hipStream_t s, size_t from, size_t to) const
{
    if (to > from) OV2_HIP_CHECK(hipMemcpyAsync(d + from, h + from, to - from, hipMemcpyHostToDevice, s));
    return OV2_OK;
}
int DevBlock::down(hipStream_t s, size_t from, size_t to) const
{
    if (to > from) OV2_HIP_CHECK(hipMemcpyAsync(h + from, d + from, to - from, hipMemcpyDeviceToHost, s));
    return OV2_OK;
}
int alloc_all(std::initializer_list<DevBlockSpec> blocks, hipStream_t s, const char *who)
{
    int rc = OV2_OK;
    for (const DevBlockSpec &q : blocks) if (rc == OV2_OK) rc = q.b->alloc(q.host_bytes, q.dev_bytes, s, who);
    if (rc != OV2_OK) for (const DevBlockSpec &q : blocks) q.b->release();
    return rc;
}

// One step as its _begin call describes it.  Each form includes the one before it: map -- the priors come from the device (wpt_h /
// is3d_h / Tcw_h; prior_xy_h / has_prior_h are unused); pose -- the pose of ov2_btracker_track_frame_pose follows in the same
// enqueue; epi -- the filter of ov2_btracker_track_frame_epi_pose runs between the pose's select and its pack.
// mono -- ov2_btracker_track_mono: the epi form (or, with doepipolar == 0, the pose form) between the motion model and the keyframe
// decision; track_frame_begin resolves it to that inner form plus Pending::mono.
struct StepArgs {
    StepForm form = STEP_PLAIN;
    int n_active = 0, stride = 0, klt_use_prior = 0;
    const uint8_t *const *img_h = nullptr;
    const float *kps_xy_h = nullptr; const int *n_h = nullptr;
    const float *prior_xy_h = nullptr; const uint8_t *has_prior_h = nullptr;                               // plain
    const double *wpt_h = nullptr; const uint8_t *is3d_h = nullptr; const double *Tcw_h = nullptr;         // map and later
    const ov2_frame_pose_params *pp = nullptr; const ov2_frame_pose_input *pin = nullptr;                  // pose (epi: the pose halves of epp / ein)
    const ov2_frame_epi_pose_params *epp = nullptr; const ov2_frame_epi_pose_input *ein = nullptr;         // epi
    const ov2_track_mono_params *mp = nullptr; const ov2_track_mono_input *min = nullptr;                  // mono (epp / ein: their step halves)
    bool resident = false;            // mono on the resident frame: n_h holds the mirror's counts, the point arrays are NULL
};

static void btracker_free(ov2_btracker *t)
{
    if (!t) return;
    if (t->ctx) { (void)hipSetDevice(t->ctx->device); (void)hipStreamSynchronize(t->ctx->stream); }
    if (t->cs) { (void)hipStreamSynchronize(t->cs); (void)hipStreamDestroy(t->cs); }
    if (t->ps) { (void)hipStreamSynchronize(t->ps); (void)hipStreamDestroy(t->ps); }
    if (t->lut) (void)hipFree(t->lut);
    for (int i = 0; i < BT_SETS; i++) {
        for (ov2_pyr *v : t->view[i]) ov2_pyr_destroy(v);
        ov2_pyr_destroy(t->pyr[i]);
    }
    for (int i = 0; i < BT_IMG_SETS; i++) {
        if (t->up_ev[i]) (void)hipEventDestroy(t->up_ev[i]);
        if (t->used_ev[i]) (void)hipEventDestroy(t->used_ev[i]);
        if (t->himg[i]) (void)hipHostFree(t->himg[i]);
        if (t->dimg[i]) (void)hipFree(t->dimg[i]);
        if (t->draw[i]) (void)hipFree(t->draw[i]);
    }
    for (ov2_pyr *v : t->kf_view) ov2_pyr_destroy(v);
    ov2_pyr_destroy(t->kf_store);
    for (IoBlock *b : {&t->pt, &t->map, &t->pose, &t->epi, &t->mono}) b->release();
    if (t->depi) (void)hipFree(t->depi);
    for (DevBlock *b : {&t->res, &t->mw, &t->work, &t->fx, &t->det, &t->out, &t->roi, &t->ckf, &t->ckw, &t->fr, &t->ctl, &t->skf, &t->anc, &t->tkf,
                        &t->ap, &t->kfpx, &t->mi})
        b->release();
    delete t;
}

// What the _begin of a call of kind `who` refuses: any open call.  name: ov2_btracker_<name>_begin / _end; sign: what this kind's
// _begin puts in front when ANOTHER kind is open.
static const struct { const char *name, *sign; } k_calls[] = {
    {nullptr, nullptr},
    {"track_frame", "ov2_btracker_track_frame_begin"},
    {"create_keyframe", "ov2_btracker_create_keyframe_begin"},
    {"stereo_keyframe", "ov2_btracker_stereo_keyframe"},
    {"temporal_keyframe", "ov2_btracker_temporal_keyframe"},
    {"mono_init", "ov2_btracker_mono_init"},
};
int begin_guard(const ov2_btracker *t, OpenCall who)
{
    const OpenCall o = t->open;
    if (o == CALL_NONE) return OV2_OK;
    const char *w = k_calls[who].name, *n = k_calls[o].name;
    if (o == who)
        ov2_set_error("%s:%d: ov2_btracker_%s_begin: the previous %s has not been finished (ov2_btracker_%s_end)", __FILE__, __LINE__, w,
                      who == CALL_STEP ? "step" : "call", w);
    else if (o == CALL_STEP) ov2_set_error("%s:%d: ov2_btracker_%s between steps only: a step is open", __FILE__, __LINE__, w);
    else ov2_set_error("%s:%d: %s: ov2_btracker_%s_begin has not been finished (ov2_btracker_%s_end)", __FILE__, __LINE__, k_calls[who].sign, n, n);
    return OV2_EINVAL;
}

// a pyramid handle that covers items [0, n) of `p` (host-side descriptor copy: the launchers size their grids from d.batch)
static inline ov2_pyr prefix_of(const ov2_pyr *p, int n) { ov2_pyr q = *p; q.d.batch = n; return q; }

// preprocessImage of items [0, n) into pyramid `dst` from dimg[which], enqueued on `on` (the caller's context, or the tracker's
// prep-stream context when the frame is prepared ahead)
static int enqueue_preprocess(ov2_btracker *t, ov2_ctx *on, ov2_pyr *dst, int which, int n)
{
    const ov2_tracker_config &c = t->cfg;
    ov2_pyr q = prefix_of(dst, n);
    int rc;
    if (t->rect) {                                                       // rectifyImage of the n raw frames, one launch
        rc = ov2_launch_remap(on->stream, t->rect, t->draw[which], t->img_pitch, t->img_bytes, n, t->dimg[which], t->img_pitch, t->img_bytes);
        if (rc != OV2_OK) return rc;
    }
    if (c.use_clahe) {
        const PyrLevelDesc &L0 = q.d.lv[0];
        int l1_done = 0;
        rc = ov2_launch_clahe(on, t->dimg[which], c.w, c.h, (int)t->img_pitch, t->img_bytes, n, c.clahe_clip, c.tiles_x, c.tiles_y,
                              q.d.base + L0.img_roi, L0.img_pitch, (size_t)q.d.item_stride, t->lut, q.d.win, &q.d, &l1_done);
        if (rc != OV2_OK) return rc;
        rc = ov2_launch_pyr_build(on, &q, nullptr, 0, 0, l1_done);
    } else
        rc = ov2_launch_pyr_build(on, &q, t->dimg[which], (int)t->img_pitch, t->img_bytes);
    if (rc != OV2_OK) return rc;
    OV2_HIP_CHECK(hipEventRecord(t->used_ev[which], on->stream));
    return OV2_OK;
}

static MonoArgs mono_args(ov2_btracker *t, const ov2_btracker::Pending &P, bool chain);           // (below, with the mono side's staging)
static int enqueue_mono_tail(ov2_btracker *t, const ov2_btracker::Pending &P, bool chain);
static int enqueue_res_stage(ov2_btracker *t, int n_active);                                      // (below: the resident frame)
static int enqueue_res_carry(ov2_btracker *t, const ov2_btracker::Pending &P);

// kltTracking of items [0, P.n_active) for the step P describes: keypoint block in, the fused LK launch, computeKeypoint, result block out
// map form: k_prior_frame fills the prior and flag slots from the map side first
// pose form: the pose set, computePose's chain and the removal bytes follow k_compute_keypoints; epi form: with the filter's hook
static int enqueue_klt(ov2_btracker *t, const ov2_pyr *prev, const ov2_pyr *cur, const ov2_btracker::Pending &P)
{
    ov2_ctx *ctx = t->ctx;
    const ov2_tracker_config &c = t->cfg;
    const hipStream_t s = ctx->stream;
    const int n = P.n_active;
    const BtPointLayout &pl = t->pl;
    const BtMapLayout &ml = t->ml;
    uint8_t *k = t->pt.k;
    const uint8_t *m = t->map.k;
    // a resident step sends the blocks' per-item headers only: k_res_stage fills the per-slot ranges behind these uploads
    const bool res = P.resident;
    int rc = res ? t->pt.upload(s, 0, pl.o_kps) : t->pt.upload(s, pl.in_bytes);  if (rc) return rc;
    if (P.form >= STEP_MAP) {
        rc = res ? t->map.upload(s, 0, ml.m_w) : t->map.upload(s, ml.map_bytes);  if (rc) return rc;
        if (P.mono) {
            // the motion model, behind the uploads of the two blocks it writes into (a mirrored block's upload would overwrite it)
            // and ahead of k_prior_frame; the filter's inputs travel here when the inner step does not take them (lmid is needed)
            rc = res ? t->pose.upload(s, 0, t->ql.q_sc) : t->pose.upload(s, t->ql.q_in);  if (rc) return rc;
            rc = t->mono.upload(s, t->nl.n_in);  if (rc) return rc;
            if (P.form != STEP_EPI) { rc = res ? t->epi.upload(s, t->el.e_nk, t->el.e_in) : t->epi.upload(s, t->el.e_in);  if (rc) return rc; }
            if (res) { rc = enqueue_res_stage(t, n);  if (rc != OV2_OK) return rc; }
            rc = ov2_launch_mono_apply(s, mono_args(t, P, true), n);
            if (rc != OV2_OK) return rc;
        }
        rc = ov2_launch_prior_frame(s, t->calib, (double)c.w, (double)c.h, P.use_prior ? 1 : 0, m + ml.m_it, (const double *)(m + ml.m_T),
                                    (const float *)(k + pl.o_kps), m + ml.m_3d, (const double *)(m + ml.m_w), (float *)(k + pl.o_pri),
                                    k + pl.o_flg, c.n_max, n);
        if (rc != OV2_OK) return rc;
    }
    if (P.from_kf) {
        // kltTrackingFromKF: `prev` is the keyframe store.  k_kf_join puts the keyframe's px where the tracking kernel reads its source
        // points and flags the slots the keyframe no longer holds; the frame's own px is the retry prior (visual_front_end.cpp:386)
        const BtEpiLayout &el = t->el;
        if (!res && P.form == STEP_EPI) { rc = t->epi.upload(s, el.e_lm, el.e_nk);  if (rc) return rc; }     // the ids, ahead of the filter's upload
        KfJoinArgs j;
        j.tab = kfpx_table(t);
        j.n_dev = (const int *)(k + pl.o_n); j.lmid = (const int *)(t->epi.k + el.e_lm);
        j.hdr = (const FeKfHdr *)t->fx.d; j.kf_lmid = (const int *)(t->depi + t->eL0.o_kl);
        j.kps = (const float2 *)(k + pl.o_kps); j.src = (float2 *)(t->kfpx.d + t->kl.w_src); j.flags = k + pl.o_flg;
        rc = ov2_launch_kf_join(s, j, n);
        if (rc != OV2_OK) return rc;
        rc = ov2_launch_track_klt_kf(s, prev, cur, c.win, c.prior_pyr_lvl, c.nklt_pyr_lvl, c.max_iter, c.eps, c.err_th, c.fb_dist, c.n_max,
                                     j.n_dev, (const float *)j.src, (const float *)(k + pl.o_pri), (const float *)(k + pl.o_kps), k + pl.o_flg,
                                     (float *)(k + pl.o_out), k + pl.o_st, nullptr, ctx->track_impl, n, ctx->lk_acc);
    } else
        rc = ov2_launch_track_klt(s, prev, cur, c.win, c.prior_pyr_lvl, c.nklt_pyr_lvl, c.max_iter, c.eps, c.err_th, c.fb_dist,
                                  c.n_max, (const int *)(k + pl.o_n), (const float *)(k + pl.o_kps), (const float *)(k + pl.o_pri),
                                  k + pl.o_flg, (float *)(k + pl.o_out), k + pl.o_st, nullptr, nullptr, 0.f, ctx->track_impl, n, ctx->lk_acc);
    if (rc != OV2_OK) return rc;
    if (t->has_calib) {
        rc = ov2_launch_compute_keypoints(s, t->calib, (const float *)(k + pl.o_out), c.n_max, (const int *)(k + pl.o_n),
                                          (float *)(k + pl.o_unpx), (double *)(k + pl.o_bv), n);
        if (rc != OV2_OK) return rc;
    }
    if (P.form >= STEP_POSE) {
        const BtPoseLayout &ql = t->ql;
        if (!P.mono) { rc = t->pose.upload(s, ql.q_in);  if (rc) return rc; }
        uint8_t *q = t->pose.k;
        bool search = P.pp.dop3p != 0;
        for (int b = 0; b < n; b++) search = search || P.req[(size_t)b];
        ov2_fp_hook hook = nullptr;
        if (P.form == STEP_EPI) {                                       // the filter between the select and the pack (frameepi.hip)
            const BtEpiLayout &el = t->el;
            rc = res ? t->epi.upload(s, el.e_nk, el.e_in) : t->epi.upload(s, el.e_in);  if (rc) return rc;
            uint8_t *e = t->epi.k, *d = t->depi;
            const EpifLayout &EL = P.eL;
            FeStep &fe = t->fe;
            FeArgs &a = fe.a;
            a.n_dev = (const int *)(k + pl.o_n); a.status = k + pl.o_st; a.is3d = m + ml.m_3d;
            a.unpx = (const float2 *)(k + pl.o_unpx); a.bv = (const double *)(k + pl.o_bv);
            a.lmid = (const int *)(e + el.e_lm); a.nbkfs = (const int *)(e + el.e_nk); a.seed = (const unsigned long long *)(e + el.e_sd);
            a.Twc = (const double *)(q + ql.q_T); a.hdr = (const FeKfHdr *)t->fx.d;
            a.items = (EpifItem *)(d + EL.o_it); a.c_lmid = (int *)(d + EL.o_lm); a.c_unpx = (float2 *)(d + EL.o_un);
            a.c_bv = (double *)(d + EL.o_bv); a.c_is3d = d + EL.o_3d;
            a.slot = (int *)(t->fx.d + el.x_slot); a.rank = (int *)(t->fx.d + el.x_rank);
            a.out = (const EpifOut *)(d + EL.o_out); a.removed = d + EL.o_rm; a.err = (const float *)(d + EL.o_er);
            a.pair_cur = (const int *)(d + EL.o_pc);
            a.sel = nullptr;
            a.out_io = (EpifOut *)(e + el.e_out); a.ncur_io = (int *)(e + el.e_nc); a.removed_io = e + el.e_rm;
            a.err_io = (float *)(e + el.e_er); a.pair_io = (int *)(e + el.e_pc);
            a.n_max = c.n_max; a.n_rows = P.ep.n_rows;
            fe.params = &P.ep; fe.L = EL; fe.block = d; fe.n_active = n;
            hook = ov2_frame_epi_hook;
        }
        FramePoseIo io;
        io.n_dev = (const int *)(k + pl.o_n); io.status = k + pl.o_st; io.unpx = (const float *)(k + pl.o_unpx); io.bv = (const double *)(k + pl.o_bv);
        io.wpt = (const double *)(m + ml.m_w); io.is3d = m + ml.m_3d;
        io.Twc = (const double *)(q + ql.q_T); io.scale = (const int *)(q + ql.q_sc); io.flags = q + ql.q_fl;
        io.seed = (const unsigned long long *)(q + ql.q_seed);
        io.work = t->work.d; io.out = (PoseOut *)(q + ql.q_out); io.ms = (int *)(q + ql.q_ms); io.removed_slot = q + ql.q_rm;
        rc = ov2_launch_frame_pose(s, &P.pp.pose, P.L, n, search, io, hook, &t->fe);
        if (rc != OV2_OK) return rc;
        rc = t->pose.download(s, ql.q_out, ql.pose_bytes);
        if (rc == OV2_OK && P.form == STEP_EPI) rc = t->epi.download(s, t->el.e_out, t->el.epi_bytes);
        if (rc == OV2_OK && P.mono) rc = enqueue_mono_tail(t, P, true);
        if (rc == OV2_OK && res) rc = enqueue_res_carry(t, P);
        if (rc != OV2_OK) return rc;
    }
    rc = t->pt.download(s, pl.o_out, pl.blk_bytes);
    if (rc == OV2_OK && P.form >= STEP_MAP) rc = t->pt.download(s, pl.o_pri, pl.in_bytes);   // the priors and flags the device set come back with the results
    return rc;
}

// Frames of items [0, n) -> dimg[which] on the main stream, `which` = the staging set the step reads.  Frames that already sit in
// a pinned slot are not copied on the host; a set uploaded ahead (ov2_btracker_upload) is only waited for; *prepared: the set was
// pre-processed ahead as well (ov2_btracker_prepare) -- nothing is enqueued for it here.
static int stage_and_upload(ov2_btracker *t, int n, const uint8_t *const *img_h, int stride, int *which_out, bool *prepared)
{
    *prepared = false;
    const int w = t->cfg.w, h = t->cfg.h;
    int which = -1;
    for (int s = 0; s < BT_IMG_SETS && which < 0; s++) {
        bool all = (size_t)stride == t->img_pitch;
        for (int b = 0; b < n && all; b++) all = img_h[b] == t->himg[s] + (size_t)b * t->img_bytes;
        if (all) which = s;
    }
    const bool in_place = which >= 0;
    if (!in_place) which = (int)(t->frames % BT_IMG_SETS);
    // the set's previous H2D (an upload started ahead, or the inline copy of an earlier step) must have left the pinned slots before
    // they are rewritten, and a pending look-ahead upload of a set that is now filled differently is void
    if (!t->prepq.empty()) {
        // frames were prepared ahead: the step must consume the oldest of them, exactly
        const ov2_btracker::Prep &pf = t->prepq.front();
        OV2_REQUIRE(in_place && pf.which == which && pf.n >= n && pf.set == (int)(t->frames % BT_SETS), OV2_EINVAL,
                    "ov2_btracker_track_frame: the frames passed are not the ones ov2_btracker_prepare was called for");
        *prepared = true; *which_out = which;
        return OV2_OK;
    }
    if (!in_place) {
        if (t->up_n[which]) { OV2_HIP_CHECK(hipEventSynchronize(t->up_ev[which])); t->up_n[which] = 0; }
        for (int b = 0; b < n; b++) {
            uint8_t *dst = t->himg[which] + (size_t)b * t->img_bytes;
            if ((size_t)stride == t->img_pitch) memcpy(dst, img_h[b], (size_t)stride * (h - 1) + (size_t)w);   // the last row holds w valid bytes only
            else for (int y = 0; y < h; y++) memcpy(dst + (size_t)y * t->img_pitch, img_h[b] + (size_t)y * stride, (size_t)w);
        }
    }
    if (in_place && t->up_n[which] >= n) OV2_HIP_CHECK(hipStreamWaitEvent(t->ctx->stream, t->up_ev[which], 0));
    else {
        if (t->up_n[which]) OV2_HIP_CHECK(hipStreamWaitEvent(t->ctx->stream, t->up_ev[which], 0));     // a shorter look-ahead copy: order after it
        OV2_HIP_CHECK(hipMemcpyAsync(t->upload_dst(which), t->himg[which], (size_t)n * t->img_bytes, hipMemcpyHostToDevice, t->ctx->stream));
    }
    t->up_n[which] = 0;
    *which_out = which;
    return OV2_OK;
}

// the map side of a step into hmap (allocated here by the first such step)
static int stage_map(ov2_btracker *t, int n_active, const double *wpt, const uint8_t *is3d, const double *Tcw, const int *n_h)
{
    const size_t nm = (size_t)t->cfg.n_max;
    if (!t->map.h) { const int rc = t->map.alloc(t->ml.map_bytes, t->zero_copy, false, "ov2_btracker_track_frame_map");  if (rc) return rc; }
    uint8_t *hmap = t->map.h;
    const BtMapLayout &ml = t->ml;
    int *it = (int *)(hmap + ml.m_it);
    for (int b = 0; b < t->batch; b++) {
        it[4 * b] = (int)((size_t)b * nm); it[4 * b + 1] = b < n_active ? n_h[b] : 0; it[4 * b + 2] = it[4 * b + 3] = 0;
    }
    if (Tcw) memcpy(hmap + ml.m_T, Tcw, 56 * (size_t)n_active);      // (mono: k_mono_apply writes the inverse of the predicted pose)
    for (int b = 0; b < n_active; b++) {
        const size_t n = (size_t)n_h[b], o = (size_t)b * nm;
        if (!n || !wpt) continue;                                        // (a resident step: k_res_stage writes both)
        memcpy(hmap + ml.m_w + 24 * o, wpt + 3 * o, 24 * n);
        memcpy(hmap + ml.m_3d + o, is3d + o, n);
        t->slot_bytes += 25 * n;
    }
    return OV2_OK;
}

// what a pose step refuses beyond the map form's checks (n_active and the counts are known to be in range); *L: the chain's layout
// mono: the pose comes from the device (Twc_h must be NULL)
static int check_pose(const ov2_btracker *t, const StepArgs &A, const ov2_frame_pose_params *pp, const ov2_frame_pose_input *in, PoseLayout *L,
                      bool mono)
{
    OV2_REQUIRE(pp && in, OV2_EINVAL, "ov2_btracker_track_frame_pose: NULL params / input");
    OV2_REQUIRE((mono ? !in->Twc_h : in->Twc_h != nullptr) && in->p3p_req_h && in->seed_h, OV2_EINVAL,
                mono ? "ov2_btracker_track_mono: Twc_h must be NULL (the pose is resident), p3p_req_h / seed_h must not"
                     : "ov2_btracker_track_frame_pose: NULL Twc_h / p3p_req_h / seed_h");
    int rc = pose_check_params(&pp->pose);  if (rc) return rc;
    OV2_REQUIRE(pp->n_rows >= 0, OV2_EINVAL, "negative count (n_rows)");
    OV2_REQUIRE(pp->n_rows <= OV2_P3P_MAX_ROWS, OV2_EINVAL, "capacity: more than 4096 sample rows in one problem");
    OV2_REQUIRE(t->cfg.n_max <= OV2_P3P_MAX_POINTS, OV2_EINVAL, "capacity: cfg.n_max exceeds the 2048 points of one pose problem");
    rc = pose_layout(t->batch, t->cfg.n_max, pp->n_rows, L);  if (rc) return rc;
    const size_t nm = (size_t)t->cfg.n_max;
    for (int b = 0; b < A.n_active; b++) {
        for (int c = 0; c < 7 && !mono; c++) OV2_REQUIRE(std::isfinite(in->Twc_h[7 * (size_t)b + c]), OV2_EINVAL, "Twc not finite");
        const size_t n = (size_t)(A.n_h ? A.n_h[b] : 0), o = (size_t)b * nm;
        for (size_t i = 0; i < n; i++) {
            if (in->scale_h) OV2_REQUIRE(in->scale_h[o + i] >= -60 && in->scale_h[o + i] <= 60, OV2_EINVAL, "|scale| > 60");
            if (A.is3d_h && A.wpt_h && A.is3d_h[o + i]) {
                const double *w = A.wpt_h + 3 * (o + i);
                OV2_REQUIRE(std::isfinite(w[0]) && std::isfinite(w[1]) && std::isfinite(w[2]), OV2_EINVAL, "wpt not finite on a 3-D slot");
            }
        }
    }
    return OV2_OK;
}

// the pose inputs of a step into hpose (the pose buffers are allocated here by the first pose step, and grown when a step asks for
// more sample rows than any before it)
static int stage_pose(ov2_btracker *t, int n_active, const ov2_frame_pose_params *pp, const ov2_frame_pose_input *in, const int *n_h,
                      const PoseLayout &L, bool resident = false)
{
    const size_t nm = (size_t)t->cfg.n_max;
    if (!t->pose.h) { const int rc = t->pose.alloc(t->ql.pose_bytes, t->zero_copy, false, "ov2_btracker_track_frame_pose");  if (rc) return rc; }
    const size_t need = ov2_frame_pose_work_bytes(L);
    if (need > t->work.dev_bytes) {
        t->lp.on = false;                                                // the lists of the last step go with the block
        const int rc = t->work.grow(need, t->ctx->stream, "ov2_btracker_track_frame_pose");  if (rc) return rc;
    }
    uint8_t *hpose = t->pose.h;
    const BtPoseLayout &ql = t->ql;
    if (in->Twc_h) memcpy(hpose + ql.q_T, in->Twc_h, 56 * (size_t)n_active);     // (mono: k_mono_apply writes the predicted pose)
    memcpy(hpose + ql.q_seed, in->seed_h, 8 * (size_t)n_active);
    uint8_t *fl = hpose + ql.q_fl;
    for (int b = 0; b < n_active; b++) {
        const int req = in->p3p_req_h[b] != 0;
        fl[b] = (uint8_t)(req | ((req || pp->dop3p) ? 2 : 0));
        const size_t n = (size_t)n_h[b], o = (size_t)b * nm;
        if (resident) continue;                                          // (k_res_stage writes the scales: all 0)
        int *sc = (int *)(hpose + ql.q_sc) + o;
        if (in->scale_h) memcpy(sc, in->scale_h + o, 4 * n); else memset(sc, 0, 4 * n);
        t->slot_bytes += 4 * n;
    }
    return OV2_OK;
}

// what an epipolar + pose step refuses beyond the pose step's checks; *L: the filter's layout at capacity
static int check_epi(const ov2_btracker *t, const ov2_frame_epi_pose_params *pp, const ov2_frame_epi_pose_input *in, EpifLayout *L,
                     bool resident = false)
{
    OV2_REQUIRE(pp && in, OV2_EINVAL, "ov2_btracker_track_frame_epi_pose: NULL params / input");
    OV2_REQUIRE((resident || in->lmid_h) && in->nbkfs_h && in->epi_seed_h, OV2_EINVAL, "ov2_btracker_track_frame_epi_pose: NULL lmid_h / nbkfs_h / epi_seed_h");
    const int rc = epif_check_params(&pp->epi);  if (rc) return rc;
    OV2_REQUIRE(t->cfg.n_max <= OV2_FKF_MAX_POINTS, OV2_EINVAL, "capacity: cfg.n_max exceeds OV2_FKF_MAX_POINTS (2048) keypoints of one frame");
    return epif_layout_capacity(t->batch, t->cfg.n_max, pp->epi.n_rows, L);
}

// The epipolar side's buffers (allocated by the first call) and the filter's block, grown to hold layout L.  The keyframe arrays lie
// in the block's input section, whose offsets do not depend on the rows: a grown block gets them again from the host copy.
int ensure_epi(ov2_btracker *t, const EpifLayout *L)
{
    const char *who = "ov2_btracker_track_frame_epi_pose";
    OV2_HIP_CHECK(hipSetDevice(t->ctx->device));
    if (!t->epi.h) {
        EpifLayout L0;
        int rc = epif_layout_capacity(t->batch, t->cfg.n_max, 0, &L0);  if (rc) return rc;
        rc = t->epi.alloc(t->el.epi_bytes, t->zero_copy, false, who);  if (rc) return rc;
        rc = t->fx.alloc(0, t->el.fx_bytes, t->ctx->stream, who);           // zeroed: no item has a keyframe yet
        if (rc) { t->epi.release(); return rc; }
        t->eL0 = L0;
        t->kf_host.assign(L0.o_up - L0.o_kl, 0);
        t->kf_hdr.assign((size_t)t->batch, FeKfHdr());
    }
    const size_t need = L ? L->total : t->eL0.total;
    if (!t->depi || need > t->depi_bytes) {
        OV2_HIP_CHECK(hipStreamSynchronize(t->ctx->stream));              // (the previous step's chain has long finished: _end waited for it)
        uint8_t *nd = nullptr;
        hipError_t e = hipMalloc((void **)&nd, need);
        if (e == hipSuccess) e = hipMemset(nd, 0, need);
        if (e == hipSuccess) e = hipMemcpy(nd + t->eL0.o_kl, t->kf_host.data(), t->kf_host.size(), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            if (nd) (void)hipFree(nd);
            (void)hipGetLastError();
            ov2_set_error("%s: %s", who, hipGetErrorString(e));
            return OV2_ENOMEM;
        }
        if (t->depi) (void)hipFree(t->depi);
        t->depi = nd; t->depi_bytes = need; t->le.on = false;           // the lists of the last step go with the block
    }
    return OV2_OK;
}

// item b's keyframe arrays in kf_host (the block's [o_kl, o_up) as the layout without rows puts them)
KfHost kf_host_item(ov2_btracker *t, int b)
{
    const EpifLayout &E = t->eL0;
    uint8_t *kh = t->kf_host.data();
    const size_t o = (size_t)b * (size_t)t->cfg.n_max;
    return KfHost{(int *)kh + o, (float *)(kh + (E.o_ku - E.o_kl)) + 2 * o, (double *)(kh + (E.o_kb - E.o_kl)) + 3 * o};
}

KfPxTable kfpx_table(const ov2_btracker *t)
{
    return KfPxTable{t->kfpx.d, t->kl.k_item, t->kl.k_lm, t->kl.k_px, t->cfg.n_max};
}

// the filter's inputs of a step into hepi
static void stage_epi(ov2_btracker *t, int n_active, const ov2_frame_epi_pose_input *in, const int *n_h)
{
    const size_t nm = (size_t)t->cfg.n_max;
    for (int b = 0; b < n_active; b++)
        if (n_h[b] > 0 && in->lmid_h) {                                   // (NULL: a resident step, k_res_stage writes the ids)
            memcpy(t->epi.h + t->el.e_lm + 4 * nm * (size_t)b, in->lmid_h + nm * (size_t)b, 4 * (size_t)n_h[b]);
            t->slot_bytes += 4 * (size_t)n_h[b];
        }
    if (in->nbkfs_h) memcpy(t->epi.h + t->el.e_nk, in->nbkfs_h, 4 * (size_t)n_active);         // (NULL: mono without the filter)
    if (in->epi_seed_h) memcpy(t->epi.h + t->el.e_sd, in->epi_seed_h, 8 * (size_t)n_active);
}

// the host mirrors of items [b0, b1) to the resident block, on the context's stream; returns when the copies are done
static int mono_push(ov2_btracker *t, int b0, int b1)
{
    const BtMonoLayout &nl = t->nl;
    const size_t o = (size_t)b0, n = (size_t)(b1 - b0);
    hipStream_t s = t->ctx->stream;
    OV2_HIP_CHECK(hipMemcpyAsync(t->res.d + nl.r_T + 56 * o, t->res_T.data() + 7 * o, 56 * n, hipMemcpyHostToDevice, s));
    OV2_HIP_CHECK(hipMemcpyAsync(t->res.d + nl.r_st + sizeof(ov2_motion_state) * o, t->res_st.data() + o, sizeof(ov2_motion_state) * n, hipMemcpyHostToDevice, s));
    OV2_HIP_CHECK(hipMemcpyAsync(t->res.d + nl.r_kt + 8 * o, t->res_kt.data() + o, 8 * n, hipMemcpyHostToDevice, s));
    OV2_HIP_CHECK(hipMemcpyAsync(t->res.d + nl.r_ki + sizeof(MonoKfInfo) * o, t->res_ki.data() + o, sizeof(MonoKfInfo) * n, hipMemcpyHostToDevice, s));
    OV2_HIP_CHECK(hipStreamSynchronize(s));
    return OV2_OK;
}

// The mono side's buffers, allocated by the first setter or step of the kind: the I/O block, the resident block with its host mirrors
// (pose: the identity; state: reset(); no keyframe info) and the work block
int ensure_mono(ov2_btracker *t)
{
    if (t->res.d) return OV2_OK;
    const char *who = "ov2_btracker_track_mono";
    OV2_HIP_CHECK(hipSetDevice(t->ctx->device));
    const size_t B = (size_t)t->batch;
    if (!t->mono.h) { const int rc = t->mono.alloc(t->nl.mono_bytes, t->zero_copy, false, who);  if (rc) return rc; }
    const int rc = alloc_all({{&t->res, 0, t->nl.res_bytes}, {&t->mw, 0, t->nl.work_bytes}}, t->ctx->stream, who);
    if (rc) return rc;
    ov2_motion_state s0;
    memset(&s0, 0, sizeof s0);
    s0.prev_time = -1.; s0.prevTwc[6] = 1.;
    t->res_st.assign(B, s0);
    t->res_T.assign(7 * B, 0.);
    for (size_t b = 0; b < B; b++) t->res_T[7 * b + 6] = 1.;
    t->res_kt.assign(B, 0.);
    t->res_ki.assign(B, MonoKfInfo{0, 0, 0, 0});
    return mono_push(t, 0, t->batch);
}

// what the five calls around the resident pose, state and keyframe info share: the item, no open step, the buffers
int mono_item(ov2_btracker *t, int item, const char *open_msg)
{
    OV2_REQUIRE(t, OV2_EINVAL, "NULL tracker");
    OV2_REQUIRE(item >= 0 && item < t->batch, OV2_EINVAL, "batch item out of range");
    OV2_REQUIRE(!t->open_call(), OV2_EINVAL, open_msg);
    return ensure_mono(t);
}

// the mono inputs of a step into the I/O block
static void stage_mono(ov2_btracker *t, const ov2_btracker::Pending &P)
{
    const size_t n = (size_t)P.n_active;
    memcpy(t->mono.h + t->nl.n_tm, P.time.data(), 8 * n);
    memcpy(t->mono.h + t->nl.n_id, P.frame_id.data(), 4 * n);
    memcpy(t->mono.h + t->nl.n_ba, P.localba.data(), 4 * n);
}

// the device pointers of a mono step (mono_dev.hpp); chain: the step's kernels ran (else every frame is empty)
static MonoArgs mono_args(ov2_btracker *t, const ov2_btracker::Pending &P, bool chain)
{
    const BtMonoLayout &nl = t->nl;
    const BtPointLayout &pl = t->pl;
    uint8_t *k = t->pt.k, *m = t->map.k, *q = t->pose.k, *e = t->epi.k, *io = t->mono.k, *r = t->res.d, *w = t->mw.d;
    MonoArgs a;
    a.r_T = (double *)(r + nl.r_T); a.r_st = (ov2_motion_state *)(r + nl.r_st); a.r_kt = (const double *)(r + nl.r_kt);
    a.r_ki = (const MonoKfInfo *)(r + nl.r_ki); a.hdr = (const FeKfHdr *)t->fx.d;
    a.time = (const double *)(io + nl.n_tm); a.frame_id = (const int *)(io + nl.n_id); a.localba = (const int *)(io + nl.n_ba);
    a.q_T = (double *)(q + t->ql.q_T); a.m_T = (double *)(m + t->ml.m_T); a.pT = (double *)(io + nl.n_pT);
    a.sa = (ov2_motion_state *)(io + nl.n_sa); a.rs = io + nl.n_rs;
    a.n_dev = (const int *)(k + pl.o_n); a.status = k + pl.o_st; a.is3d = m + t->ml.m_3d;
    a.out_xy = (const float2 *)(k + pl.o_out); a.unpx = (const float2 *)(k + pl.o_unpx); a.bv = (const double *)(k + pl.o_bv);
    a.lmid = (const int *)(e + t->el.e_lm);
    a.epi_removed = chain && P.form == STEP_EPI ? e + t->el.e_rm : nullptr;
    a.pose_removed = q + t->ql.q_rm; a.pose_out = chain ? (const PoseOut *)(q + t->ql.q_out) : nullptr;
    a.items = (FkfItemD *)(w + nl.w_it); a.c_lmid = (int *)(w + nl.w_lm); a.c_px = (float2 *)(w + nl.w_px); a.c_unpx = (float2 *)(w + nl.w_un);
    a.c_bv = (double *)(w + nl.w_bv); a.c_is3d = w + nl.w_3d; a.ncur_io = (int *)(io + nl.n_nc); a.su = (ov2_motion_state *)(io + nl.n_su);
    a.n_max = t->cfg.n_max;
    return a;
}

// behind the step's kernels (or, with chain == false, behind k_mono_apply alone): the frame checkNewKfReq sees, the model's update,
// k_fkf_parallax on that frame against the resident keyframes, and the mono results on their way back
static int enqueue_mono_tail(ov2_btracker *t, const ov2_btracker::Pending &P, bool chain)
{
    const hipStream_t s = t->ctx->stream;
    const BtMonoLayout &nl = t->nl;
    const MonoArgs a = mono_args(t, P, chain);
    int rc = ov2_launch_mono_pack(s, a, P.n_active);
    if (rc != OV2_OK) return rc;
    rc = ov2_launch_kf_decision(s, &P.fkf, P.n_active, a.items, a.c_lmid, a.c_px, a.c_unpx, a.c_bv, a.c_is3d,
                                (const int *)(t->depi + t->eL0.o_kl), (const float2 *)(t->depi + t->eL0.o_ku), (int *)(t->mono.k + nl.n_dec));
    if (rc != OV2_OK) return rc;
    return t->mono.download(s, nl.n_in, nl.mono_bytes);
}

// a mono step in which no item carries a keypoint (not the first frame): the motion model and the decision run all the same
static int enqueue_mono_empty(ov2_btracker *t, const ov2_btracker::Pending &P)
{
    const hipStream_t s = t->ctx->stream;
    int rc = t->map.upload(s, t->ml.map_bytes);  if (rc) return rc;
    rc = t->pose.upload(s, t->ql.q_in);  if (rc) return rc;
    rc = t->mono.upload(s, t->nl.n_in);  if (rc) return rc;
    rc = ov2_launch_mono_apply(s, mono_args(t, P, false), P.n_active);
    if (rc != OV2_OK) return rc;
    return enqueue_mono_tail(t, P, false);
}

static void stage_points(ov2_btracker *t, int n_active, const float *kps, const float *pri, const uint8_t *has_prior, const int *n_h, int use_prior)
{
    const size_t nm = (size_t)t->cfg.n_max;
    uint8_t *hblk = t->pt.h;
    const BtPointLayout &pl = t->pl;
    int *nd = (int *)(hblk + pl.o_n);
    for (int b = 0; b < t->batch; b++) nd[b] = b < n_active ? n_h[b] : 0;
    for (int b = 0; b < n_active; b++) {
        const size_t n = (size_t)n_h[b], o = (size_t)b * nm;
        if (!n || !kps) continue;                                        // (NULL: a resident step, k_res_stage writes the keypoints)
        memcpy(hblk + pl.o_kps + 8 * o, kps + 2 * o, 8 * n);
        t->slot_bytes += 8 * n;
        if (!pri) continue;                                              // the map form: k_prior_frame writes both
        memcpy(hblk + pl.o_pri + 8 * o, pri + 2 * o, 8 * n);
        uint8_t *f = hblk + pl.o_flg + o;
        if (use_prior && has_prior) for (size_t i = 0; i < n; i++) f[i] = has_prior[o + i] ? 1 : 0;
        else memset(f, 0, n);
        t->slot_bytes += 9 * n;
    }
}

// ---- the resident frame (f21) ------------------------------------------------------------------------------------------------------
ResHost res_host(const ov2_btracker *t, int b, int other)
{
    const BtResLayout &L = t->rl;
    uint8_t *p = t->fr.h + (size_t)(t->res_sel[(size_t)b] ^ other) * L.buf_bytes + (size_t)b * L.f_item;
    return ResHost{(int *)p, (float *)(p + L.f_px), (int *)(p + L.f_lm), p + L.f_3d, (double *)(p + L.f_w)};
}

ResFrames res_frames(const ov2_btracker *t)
{
    const BtResLayout &L = t->rl;
    return ResFrames{t->fr.d, L.buf_bytes, L.f_item, L.f_px, L.f_lm, L.f_3d, L.f_w, t->ctl.d + L.u_sel, t->cfg.n_max};
}

// the frame block, its mirror and the control block, allocated by the first use: every frame empty
int ensure_res(ov2_btracker *t)
{
    if (t->fr.d) return OV2_OK;
    const char *who = "ov2_btracker_set_frame";
    OV2_REQUIRE(t->cfg.n_max <= OV2_FKF_MAX_POINTS, OV2_EINVAL, "capacity: cfg.n_max exceeds OV2_FKF_MAX_POINTS (2048) keypoints of one frame");
    OV2_HIP_CHECK(hipSetDevice(t->ctx->device));
    const BtResLayout &L = t->rl;
    const int rc = alloc_all({{&t->fr, L.frame_bytes, L.frame_bytes}, {&t->ctl, L.ctl_bytes, L.ctl_bytes}}, t->ctx->stream, who);
    if (rc) return rc;
    t->res_sel.assign((size_t)t->batch, 0);
    t->res_iskf.assign((size_t)t->batch, 0);
    return OV2_OK;
}

// which buffer holds each item's current frame, to the device (one byte per item)
int res_push_sel(ov2_btracker *t, hipStream_t s)
{
    memcpy(t->ctl.h + t->rl.u_sel, t->res_sel.data(), (size_t)t->batch);
    return t->ctl.up(s, t->rl.u_sel, t->rl.u_sel + (size_t)t->batch);
}

// item b's frame in the mirror (its current one, or with other == 1 the next one) to the same place on the device
static int res_push_item(ov2_btracker *t, int b, int other, hipStream_t s)
{
    const BtResLayout &L = t->rl;
    const size_t o = (size_t)(t->res_sel[(size_t)b] ^ other) * L.buf_bytes + (size_t)b * L.f_item;
    return t->fr.up(s, o, o + L.f_item);
}

// A resident step on mirrored blocks: what _end reads on the host again (the rule's keypoints, the re-run's points, ids and
// scales) from the mirror into the host halves of the blocks.  Nothing of it is copied up: k_res_stage writes the device halves.
// (With zero copy the kernel's writes land in these very ranges.)
static void res_fill_host(ov2_btracker *t, int n_active)
{
    const size_t nm = (size_t)t->cfg.n_max;
    for (int b = 0; b < n_active; b++) {
        const ResHost f = res_host(t, b, 0);
        const size_t n = (size_t)*f.n, o = (size_t)b * nm;
        if (!n) continue;
        memcpy(t->pt.h + t->pl.o_kps + 8 * o, f.px, 8 * n);
        memcpy(t->map.h + t->ml.m_w + 24 * o, f.wpt, 24 * n);
        memcpy(t->map.h + t->ml.m_3d + o, f.is3d, n);
        memcpy(t->epi.h + t->el.e_lm + 4 * o, f.lmid, 4 * n);
        memset(t->pose.h + t->ql.q_sc + 4 * o, 0, 4 * n);
    }
}

// in front of a resident step's kernels: which buffers are current, then the frames into the step's blocks
static int enqueue_res_stage(ov2_btracker *t, int n_active)
{
    const hipStream_t s = t->ctx->stream;
    const int rc = res_push_sel(t, s);
    if (rc != OV2_OK) return rc;
    ResStageArgs a;
    a.f = res_frames(t);
    a.kps = (float2 *)(t->pt.k + t->pl.o_kps); a.wpt = (double *)(t->map.k + t->ml.m_w); a.is3d = t->map.k + t->ml.m_3d;
    a.lmid = (int *)(t->epi.k + t->el.e_lm); a.scale = (int *)(t->pose.k + t->ql.q_sc);
    return ov2_launch_res_stage(s, a, n_active);
}

// behind k_mono_pack: the frame the step leaves into each item's other buffer, and those buffers down into the mirror (one copy
// per buffer that takes part: the items' frames are contiguous)
static int enqueue_res_carry(ov2_btracker *t, const ov2_btracker::Pending &P)
{
    const hipStream_t s = t->ctx->stream;
    const MonoArgs m = mono_args(t, P, true);
    ResCarryArgs a;
    a.f = res_frames(t);
    a.n_dev = m.n_dev; a.status = m.status; a.epi_removed = m.epi_removed; a.pose_removed = m.pose_removed; a.pose_out = m.pose_out;
    a.out_xy = m.out_xy; a.lmid = m.lmid; a.is3d = m.is3d; a.wpt = (const double *)(t->map.k + t->ml.m_w);
    const int rc = ov2_launch_res_carry(s, a, P.n_active);
    if (rc != OV2_OK) return rc;
    const BtResLayout &L = t->rl;
    for (int buf = 0; buf < 2; buf++) {
        int lo = -1, hi = -1;
        for (int b = 0; b < P.n_active; b++)
            if ((t->res_sel[(size_t)b] ^ 1) == buf) { if (lo < 0) lo = b; hi = b; }
        if (lo < 0) continue;
        // (an item in [lo, hi] whose CURRENT frame lies in this buffer is copied too: the mirror holds the same bytes)
        const size_t o = (size_t)buf * L.buf_bytes + (size_t)lo * L.f_item;
        const int rcd = t->fr.down(s, o, o + (size_t)(hi - lo + 1) * L.f_item);  if (rcd != OV2_OK) return rcd;
    }
    return OV2_OK;
}

// The resident half of _end, behind mono_finish (mres != NULL: a dropped step leaves every frame as it was).  The next frames came
// down with the results; for the items the rule re-ran (redo) the frame is rebuilt here from the second run's removals, by
// k_mono_pack's rule as mono_finish applies it, and copied up.  Then each item's other buffer becomes its current one.
static int res_finish(ov2_btracker *t, const float *out_xy_h, const uint8_t *status_h, const ov2_pose_result *results,
                      const std::vector<int> &redo, const std::vector<uint8_t> &excl, ov2_resident_step_result *fres)
{
    const ov2_btracker::Pending &P = t->pend;
    const size_t nm = (size_t)t->cfg.n_max;
    if (!P.tracked) {                                                    // the first frame, or no keypoint anywhere: nothing ran
        for (int b = 0; b < P.n_active && fres; b++) fres[b].n_before = fres[b].n_after = P.n[(size_t)b];
        return OV2_OK;
    }
    for (size_t k = 0; k < redo.size(); k++) {
        const int b = redo[k];
        const size_t o = (size_t)b * nm;
        const ov2_pose_result &pr = results[b];
        const bool reset = pr.action == OV2_POSE_P3P_RESET || pr.action == OV2_POSE_PNP_RESET;              // resetFrame()
        const int n = reset ? 0 : P.n[(size_t)b];
        const ResHost src = res_host(t, b, 0), dst = res_host(t, b, 1);
        int r = 0;
        for (int i = 0; i < n; i++)
            if ((status_h[o + i] & 3) == 1 && !(!excl.empty() && excl[o + i]) && !pr.removed[i]) {
                dst.px[2 * r] = out_xy_h[2 * (o + i)]; dst.px[2 * r + 1] = out_xy_h[2 * (o + i) + 1];
                dst.lmid[r] = src.lmid[i]; dst.is3d[r] = src.is3d[i] ? 1 : 0;
                for (int c = 0; c < 3; c++) dst.wpt[3 * r + c] = src.wpt[3 * i + c];
                r++;
            }
        *dst.n = r;
        const int rc = res_push_item(t, b, 1, t->ctx->stream);
        if (rc != OV2_OK) return rc;
    }
    if (!redo.empty()) OV2_HIP_CHECK(hipStreamSynchronize(t->ctx->stream));
    for (int b = 0; b < P.n_active; b++) {
        t->res_sel[(size_t)b] ^= 1;
        t->res_iskf[(size_t)b] = 0;                                      // the frame has moved on from its keyframe
        if (fres) { fres[b].n_before = P.n[(size_t)b]; fres[b].n_after = *res_host(t, b, 0).n; }
    }
    return OV2_OK;
}

// mode 0: detectGridFAST, 1: detectSingleScale, 2: detectGFTT (roi_h / roi_stride / gp / nbmax_h; cell unused)
static int detect_common(ov2_btracker *t, int mode, int n_active, int cell, const float *cur_xy_h, const int *ncur_h, const int roi[4],
                         double *quality_inout, int *fast_th_inout, int mask_mode, int do_subpix, float *out_xy_h, int out_cap, int *out_n_h,
                         const uint8_t *roi_h = nullptr, int roi_stride = 0, const ov2_gftt_params *gp = nullptr, const int *nbmax_h = nullptr)
{
    OV2_REQUIRE(t && out_xy_h && out_n_h, OV2_EINVAL, "NULL argument");
    OV2_REQUIRE(n_active >= 1 && n_active <= t->batch, OV2_EINVAL, "n_active out of range");
    OV2_REQUIRE(t->frames > 0, OV2_EINVAL, "no frame has been preprocessed yet");
    OV2_REQUIRE(mode == 2 || (cell >= 8 && out_cap >= (mode == 0 ? 1 : 2) * (t->cfg.w / cell) * (t->cfg.h / cell)), OV2_EINVAL, "out_cap too small for this cell size");
    OV2_REQUIRE(mode != 2 || out_cap >= 1, OV2_EINVAL, "out_cap < 1");
    ov2_ctx *ctx = t->ctx;
    OV2_HIP_CHECK(hipSetDevice(ctx->device));
    const size_t nm = (size_t)t->cfg.n_max, o_cur = up256(4 * (size_t)t->batch);
    int *nh = (int *)t->det.h;
    for (int b = 0; b < n_active; b++) {
        const int n = ncur_h ? ncur_h[b] : 0;
        OV2_REQUIRE(n >= 0 && (size_t)n <= nm && (n == 0 || cur_xy_h), OV2_EINVAL, "bad current keypoints");
        nh[b] = n;
        if (n) memcpy(t->det.h + o_cur + 8 * nm * b, cur_xy_h + 2 * nm * b, 8 * (size_t)n);
    }
    if (out_cap > t->out_cap) {                                          // grow-only result mirrors
        OV2_HIP_CHECK(hipStreamSynchronize(ctx->stream));
        t->out_cap = 0;
        const int rca = t->out.alloc(8 * (size_t)out_cap * t->batch, 8 * (size_t)out_cap * t->batch, ctx->stream, "ov2_btracker_detect");
        if (rca) return rca;
        t->out_cap = out_cap;
    }
    int rc = t->det.up(ctx->stream, 0, o_cur + 8 * nm * (size_t)n_active);  if (rc != OV2_OK) return rc;
    const ov2_pyr q = prefix_of(t->pyr[t->cur], n_active);
    const float *cur_d = (const float *)(t->det.d + o_cur);
    const int *ncur_d = (const int *)t->det.d;
    if (mode == 2 && roi_h) {
        OV2_REQUIRE(roi_stride >= t->cfg.w, OV2_EINVAL, "roi stride < width");
        if (!t->roi.d) { const int rca = t->roi.alloc(0, (size_t)t->cfg.w * t->cfg.h, ctx->stream, "ov2_btracker_detect_gftt");  if (rca) return rca; }
        OV2_HIP_CHECK(hipMemcpy2DAsync(t->roi.d, (size_t)t->cfg.w, roi_h, (size_t)roi_stride, (size_t)t->cfg.w, (size_t)t->cfg.h,
                                       hipMemcpyHostToDevice, ctx->stream));
    }
    if (mode == 2) rc = ov2_detect_gftt_batch_d(ctx, &q, roi_h ? t->roi.d : nullptr, t->cfg.w, gp, cur_d, (int)nm, ncur_d, nbmax_h, do_subpix,
                                                (float *)t->out.d, t->out_cap, out_n_h);
    else if (mode == 0) rc = ov2_detect_grid_fast_batch_d(ctx, &q, cell, cur_d, (int)nm, ncur_d, fast_th_inout, mask_mode, do_subpix, (float *)t->out.d, t->out_cap, out_n_h);
    else rc = ov2_detect_singlescale_batch_d(ctx, &q, cell, cur_d, (int)nm, ncur_d, roi, quality_inout, do_subpix, (float *)t->out.d, t->out_cap, out_n_h);
    if (rc != OV2_OK) return rc;
    rc = t->out.down(ctx->stream, 0, 8 * (size_t)t->out_cap * n_active);  if (rc != OV2_OK) return rc;
    OV2_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    for (int b = 0; b < n_active; b++)
        if (out_n_h[b] > 0) memcpy(out_xy_h + 2 * (size_t)out_cap * b, t->out.h + 8 * (size_t)t->out_cap * b, 8 * (size_t)out_n_h[b]);
    return OV2_OK;
}

extern "C" {

int ov2_btracker_create(ov2_ctx *ctx, const ov2_tracker_config *cfg, int batch, ov2_btracker **out)
{
    OV2_REQUIRE(ctx && cfg && out, OV2_EINVAL, "NULL argument");
    *out = nullptr;
    OV2_REQUIRE(batch >= 1 && batch <= 65535, OV2_EINVAL, "batch out of range");
    OV2_REQUIRE(cfg->w > 0 && cfg->h > 0 && cfg->n_max > 0 && cfg->nklt_pyr_lvl >= 0 && cfg->prior_pyr_lvl >= 0, OV2_EINVAL, "bad tracker geometry");
    OV2_REQUIRE(!cfg->use_clahe || (cfg->tiles_x > 0 && cfg->tiles_y > 0 && cfg->tiles_x <= cfg->w && cfg->tiles_y <= cfg->h), OV2_EINVAL, "bad CLAHE tiles");
    OV2_HIP_CHECK(hipSetDevice(ctx->device));
    ov2_btracker *t = new (std::nothrow) ov2_btracker();
    OV2_REQUIRE(t != nullptr, OV2_ENOMEM, "out of host memory");
    t->ctx = ctx; t->cfg = *cfg; t->batch = batch;
    t->last_n.assign((size_t)batch, 0);
    t->last_pn.assign((size_t)batch, 0);
    int rc = OV2_OK;
    for (int i = 0; i < BT_SETS && rc == OV2_OK; i++) {
        rc = ov2_pyr_create(ctx, cfg->w, cfg->h, cfg->win, cfg->nklt_pyr_lvl, batch, &t->pyr[i]);
        for (int b = 0; b < batch && rc == OV2_OK; b++) {
            ov2_pyr *v = nullptr;
            rc = ov2_pyr_item_view(t->pyr[i], b, &v);
            if (rc == OV2_OK) t->view[i].push_back(v);
        }
    }
    if (rc != OV2_OK) { btracker_free(t); return rc; }
    t->img_pitch = bt_img_pitch(cfg->w);
    t->img_bytes = bt_img_bytes(cfg->w, cfg->h);
    t->pl = bt_point_layout(batch, cfg->n_max); t->ml = bt_map_layout(batch, cfg->n_max);
    t->ql = bt_pose_layout(batch, cfg->n_max); t->el = bt_epi_layout(batch, cfg->n_max); t->nl = bt_mono_layout(batch, cfg->n_max);
    t->cl = bt_ckf_layout(batch, cfg->n_max); t->rl = bt_res_layout(batch, cfg->n_max); t->kl = bt_kfpx_layout(batch, cfg->n_max);
    hipError_t e = hipSuccess;
    for (int i = 0; i < BT_IMG_SETS && e == hipSuccess; i++) {
        e = hipHostMalloc((void **)&t->himg[i], t->img_bytes * batch + 256, hipHostMallocDefault);
        if (e == hipSuccess) e = hipMalloc((void **)&t->dimg[i], t->img_bytes * batch + 256);
        if (e == hipSuccess) e = hipMemsetAsync(t->dimg[i], 0, t->img_bytes * batch + 256, ctx->stream);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&t->up_ev[i], hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&t->used_ev[i], hipEventDisableTiming);
        if (e == hipSuccess) memset(t->himg[i], 0, t->img_bytes * batch + 256);
    }
    {   // the look-ahead streams inherit the priority of the context's stream
        int prio = 0;
        if (e == hipSuccess) e = hipStreamGetPriority(ctx->stream, &prio);
        if (e == hipSuccess) e = hipStreamCreateWithPriority(&t->cs, hipStreamNonBlocking, prio);
        if (e == hipSuccess) e = hipStreamCreateWithPriority(&t->ps, hipStreamNonBlocking, prio);
    }
    if (e == hipSuccess) e = hipMalloc((void **)&t->lut, (size_t)batch * (cfg->use_clahe ? (size_t)cfg->tiles_x * cfg->tiles_y : 1) * 256 + 256);
    // the kernels read / write the pinned point block through its device alias (no staging copies); a device mirror is the fallback
    if (e == hipSuccess && (rc = t->pt.alloc(t->pl.blk_bytes, t->zero_copy, true, "ov2_btracker_create")) != OV2_OK) { btracker_free(t); return rc; }
    if (e == hipSuccess && t->pt.d) e = hipMemsetAsync(t->pt.d, 0, t->pl.blk_bytes, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) { ov2_set_error("ov2_btracker_create: %s", hipGetErrorString(e)); btracker_free(t); return OV2_ENOMEM; }
    const size_t det_in = bt_det_in_bytes(batch, cfg->n_max);
    if ((rc = t->det.alloc(det_in, det_in, ctx->stream, "ov2_btracker_create")) != OV2_OK) { btracker_free(t); return rc; }
    t->side.device = ctx->device; t->side.stream = t->ps; t->side.owns_stream = false;
    *out = t;
    return OV2_OK;
}

void ov2_btracker_destroy(ov2_btracker *t) { btracker_free(t); }
int ov2_btracker_batch(const ov2_btracker *t) { return t ? t->batch : 0; }
int ov2_btracker_frames(const ov2_btracker *t) { return t ? (int)t->frames : 0; }

uint8_t *ov2_btracker_image_buffer(ov2_btracker *t, int which, int item, int *stride)
{
    if (!t || which < 0 || which >= BT_IMG_SETS || item < 0 || item >= t->batch) return nullptr;
    if (stride) *stride = (int)t->img_pitch;
    return t->himg[which] + (size_t)item * t->img_bytes;
}

int ov2_btracker_upload(ov2_btracker *t, int which, int n_active)
{
    OV2_REQUIRE(t && which >= 0 && which < BT_IMG_SETS, OV2_EINVAL, "bad staging set");
    OV2_REQUIRE(n_active >= 1 && n_active <= t->batch, OV2_EINVAL, "n_active out of range");
    OV2_HIP_CHECK(hipSetDevice(t->ctx->device));
    if (which == t->raw_which) t->raw_which = -1;                       // the current step's raw frames are overwritten
    OV2_HIP_CHECK(hipStreamWaitEvent(t->cs, t->used_ev[which], 0));      // the step that read dimg[which] last (no-op before the first record)
    OV2_HIP_CHECK(hipMemcpyAsync(t->upload_dst(which), t->himg[which], (size_t)n_active * t->img_bytes, hipMemcpyHostToDevice, t->cs));
    OV2_HIP_CHECK(hipEventRecord(t->up_ev[which], t->cs));
    t->up_n[which] = n_active;
    return OV2_OK;
}

int ov2_btracker_prepare(ov2_btracker *t, int which, int n_active)
{
    OV2_REQUIRE(t && which >= 0 && which < BT_IMG_SETS, OV2_EINVAL, "bad staging set");
    OV2_REQUIRE(n_active >= 1 && n_active <= t->batch, OV2_EINVAL, "n_active out of range");
    OV2_REQUIRE(t->prepq.size() < 2, OV2_EINVAL, "two prepared frames are already waiting for their ov2_btracker_track_frame");
    OV2_HIP_CHECK(hipSetDevice(t->ctx->device));
    if (which == t->raw_which) t->raw_which = -1;
    // the frames: uploaded ahead (wait for the copy stream) or copied here, on the prep stream
    if (t->up_n[which] >= n_active) OV2_HIP_CHECK(hipStreamWaitEvent(t->ps, t->up_ev[which], 0));
    else {
        if (t->up_n[which]) OV2_HIP_CHECK(hipStreamWaitEvent(t->ps, t->up_ev[which], 0));
        OV2_HIP_CHECK(hipStreamWaitEvent(t->ps, t->used_ev[which], 0));
        OV2_HIP_CHECK(hipMemcpyAsync(t->upload_dst(which), t->himg[which], (size_t)n_active * t->img_bytes, hipMemcpyHostToDevice, t->ps));
    }
    t->up_n[which] = 0;
    // target: the pyramid set of frame pre_count.  Its last readers on the context's stream -- the tracking kernels of the step that
    // had it as prev_pyr_ -- finished before that step's synchronisation (at most two frames are ever ahead of the tracked one);
    // consumers on other contexts are the caller's to wait for (ov2_btracker_pyramid_sets)
    const int set = (int)(t->pre_count % BT_SETS);
    t->side.clahe_strips = t->ctx->clahe_strips;
    int rc = enqueue_preprocess(t, &t->side, t->pyr[set], which, n_active);
    if (rc != OV2_OK) return rc;
    rc = ov2_pyr_mark_ready(&t->side, t->pyr[set]);
    if (rc != OV2_OK) return rc;
    t->prepq.push_back({which, n_active, set});
    t->pre_count++;
    return OV2_OK;
}

int ov2_btracker_set_calibration(ov2_btracker *t, int model, const double K[4], const double *D, int nD, const double iK[9])
{
    OV2_REQUIRE(t, OV2_EINVAL, "NULL tracker");
    KpCalib c;
    const int rc = ov2_kp_calib(model, K, D, nD, iK, c);
    if (rc != OV2_OK) return rc;
    t->calib = c; t->has_calib = true;
    return OV2_OK;
}

int ov2_btracker_set_rectification(ov2_btracker *t, const ov2_rectmap *map)
{
    OV2_REQUIRE(t, OV2_EINVAL, "NULL tracker");
    OV2_REQUIRE(!map || (map->w == t->cfg.w && map->h == t->cfg.h), OV2_EINVAL, "map and tracker differ in size");
    OV2_REQUIRE(!map || map->device == t->ctx->device, OV2_EINVAL, "the map lives on another device");
    OV2_REQUIRE(t->prepq.empty() && !t->open_call(), OV2_EINVAL, "ov2_btracker_set_rectification between steps only: prepared frames wait or a step is open");
    OV2_HIP_CHECK(hipSetDevice(t->ctx->device));
    OV2_HIP_CHECK(hipStreamSynchronize(t->cs));
    OV2_HIP_CHECK(hipStreamSynchronize(t->ps));
    OV2_HIP_CHECK(hipStreamSynchronize(t->ctx->stream));
    for (int i = 0; i < BT_IMG_SETS && map; i++)
        if (!t->draw[i]) {
            OV2_HIP_CHECK(hipMalloc((void **)&t->draw[i], t->img_bytes * t->batch + 256));
            OV2_HIP_CHECK(hipMemset(t->draw[i], 0, t->img_bytes * t->batch + 256));
        }
    // an upload started ahead went where the old setting put it: void it (the pinned slots still hold the frames; the step or the
    // prepare call that consumes them copies them again, in order)
    for (int i = 0; i < BT_IMG_SETS; i++) t->up_n[i] = 0;
    t->rect = map;
    return OV2_OK;
}

} // extern "C"

// the step's first half, for every form (StepArgs)
static int track_frame_begin(ov2_btracker *t, const StepArgs &A)
{
    const int n_active = A.n_active;
    const int *n_h = A.n_h;
    const bool mono = A.form == STEP_MONO;
    OV2_REQUIRE(!mono || (A.mp && A.min), OV2_EINVAL, "ov2_btracker_track_mono: NULL params / input");
    const StepForm form = mono ? (A.mp->doepipolar ? STEP_EPI : STEP_POSE) : A.form;         // the inner step
    const bool map = form >= STEP_MAP, pose = form >= STEP_POSE, epi = form == STEP_EPI;
    const ov2_frame_epi_pose_params *epp = mono ? &A.mp->step : A.epp;
    const ov2_frame_epi_pose_input *ein = mono ? &A.min->step : A.ein;
    OV2_REQUIRE(t && A.img_h, OV2_EINVAL, "NULL argument");
    OV2_REQUIRE(!map || t->has_calib, OV2_EINVAL, "ov2_btracker_track_frame_map: no calibration set on this tracker");
    { const int rco = begin_guard(t, CALL_STEP);  if (rco != OV2_OK) return rco; }
    OV2_REQUIRE(n_active >= 1 && n_active <= t->batch, OV2_EINVAL, "n_active out of range");
    OV2_REQUIRE(A.stride >= t->cfg.w, OV2_EINVAL, "stride < width");
    const size_t nm = (size_t)t->cfg.n_max;
    int n_total = 0;
    for (int b = 0; b < n_active; b++) {
        OV2_REQUIRE(A.img_h[b] != nullptr, OV2_EINVAL, "NULL frame of an active item");
        const int n = n_h ? n_h[b] : 0;
        OV2_REQUIRE(n >= 0 && (size_t)n <= nm, OV2_EINVAL, "an item carries more keypoints than cfg.n_max slots");
        n_total += n;
    }
    if (t->from_kf) {
        // kltTrackingFromKF joins the frame with its keyframe by lmid, and tracks from the keyframe's pyramid (the reference's
        // `pkf == nullptr` early return, visual_front_end.cpp:308-310, is a refusal here)
        OV2_REQUIRE(epi || mono, OV2_EINVAL, "the tracker tracks from the keyframe (ov2_btracker_set_track_from_keyframe): this form of the step carries no lmid");
        for (int b = 0; b < n_active && t->frames > 0; b++)
            OV2_REQUIRE(!(n_h && n_h[b] > 0) || t->kf_has_pyr[(size_t)b], OV2_EINVAL,
                        "the tracker tracks from the keyframe: an item with keypoints has no adopted keyframe pyramid");
    }
    if (map) OV2_REQUIRE(n_total == 0 || A.resident || (A.kps_xy_h && A.wpt_h && A.is3d_h && (mono || A.Tcw_h) && n_h), OV2_EINVAL, "NULL point buffer");
    else OV2_REQUIRE(n_total == 0 || (A.kps_xy_h && A.prior_xy_h && n_h), OV2_EINVAL, "NULL point buffer");
    const ov2_frame_pose_params *pp = A.pp;
    const ov2_frame_pose_input *pin = A.pin;
    PoseLayout poseL;
    EpifLayout epiL;
    if (epi || mono) {                                                   // (pp / pin: the pose halves of epp / ein)
        OV2_REQUIRE(epp && ein, OV2_EINVAL, "ov2_btracker_track_frame_epi_pose: NULL params / input");
        pp = &epp->pose; pin = &ein->pose;
    }
    if (pose) { const int rcp = check_pose(t, A, pp, pin, &poseL, mono);  if (rcp != OV2_OK) return rcp; }
    if (epi) { const int rce = check_epi(t, epp, ein, &epiL, A.resident);  if (rce != OV2_OK) return rce; }
    if (mono) {
        // what the mono step refuses of its own.  The predicted pose cannot be checked on the host: the resident pose and state are
        // finite (the setters refuse anything else, the kernels' results derive from finite ones) and dt > 0, so log and exp are finite
        OV2_REQUIRE(A.mp->doepipolar == 0 || A.mp->doepipolar == 1, OV2_EINVAL, "doepipolar is not 0 or 1");
        OV2_REQUIRE(A.resident || ein->lmid_h, OV2_EINVAL, "ov2_btracker_track_mono: NULL lmid_h");
        OV2_REQUIRE(A.min->time_h && A.min->frame_id_h, OV2_EINVAL, "ov2_btracker_track_mono: NULL time_h / frame_id_h");
        OV2_REQUIRE(t->cfg.n_max <= OV2_FKF_MAX_POINTS, OV2_EINVAL, "capacity: cfg.n_max exceeds OV2_FKF_MAX_POINTS (2048) keypoints of one frame");
        const int rcd = fkf_check_decide(&epp->epi.fkf);  if (rcd != OV2_OK) return rcd;
        for (int b = 0; b < n_active; b++) {
            const double tm = A.min->time_h[b], prev = t->res_st.empty() ? -1. : t->res_st[(size_t)b].prev_time;
            OV2_REQUIRE(std::isfinite(tm), OV2_EINVAL, "time not finite");
            OV2_REQUIRE(!(prev >= 0. && tm <= prev), OV2_EINVAL, "ov2_btracker_track_mono: time_h is not after the item's prev_time");
        }
    }
    for (int b = 0; b < t->batch; b++) t->last_n[(size_t)b] = t->last_pn[(size_t)b] = 0;
    t->slot_bytes = 0;
    ov2_ctx *ctx = t->ctx;
    OV2_HIP_CHECK(hipSetDevice(ctx->device));
    if (mono) { const int rcm = ensure_mono(t);  if (rcm != OV2_OK) return rcm; }
    int which = 0;
    bool prepared = false;
    t->raw_which = -1;                                                   // staging may rewrite any set
    int rc = stage_and_upload(t, n_active, A.img_h, A.stride, &which, &prepared);
    if (rc != OV2_OK) return rc;
    // preprocessImage: already under way on the prep stream (the context's stream waits for the pyramids' event), or in order here
    const int old_cur = t->cur;
    // the bookkeeping (prepq / pre_count) is committed only when the whole step has been enqueued: a failure further down leaves
    // the tracker where it was, and the same frames can be passed again
    auto preprocess = [&]() -> int {
        if (prepared) return ov2_pyr_wait_ready(ctx, t->pyr[t->cur]);
        const int rcp = enqueue_preprocess(t, ctx, t->pyr[t->cur], which, n_active);
        if (rcp != OV2_OK) return rcp;
        return ov2_pyr_mark_ready(ctx, t->pyr[t->cur]);
    };
    auto commit = [&]() { if (prepared) t->prepq.pop_front(); else t->pre_count++; t->frames++; t->raw_which = which; t->raw_n = n_active; };
    t->cur = (int)(t->frames % BT_SETS);                                 // prev_pyr_.swap(cur_pyr_)  (:1169): frame k lives in set k % BT_SETS
    ov2_btracker::Pending &P = t->pend;
    P.form = form; P.n_active = n_active; P.use_prior = A.klt_use_prior; P.kps = A.kps_xy_h; P.has_prior = A.has_prior_h;
    P.n.assign((size_t)n_active, 0);
    if (n_h) for (int b = 0; b < n_active; b++) P.n[(size_t)b] = n_h[b];
    if (pose) {
        P.pp = *pp; P.L = poseL;
        if (mono) P.Twc.assign(7 * (size_t)n_active, 0.);                // (the predicted poses: _end reads them back)
        else P.Twc.assign(pin->Twc_h, pin->Twc_h + 7 * (size_t)n_active);
        P.req.assign(pin->p3p_req_h, pin->p3p_req_h + n_active);
        P.seed.assign(pin->seed_h, pin->seed_h + n_active);
    }
    if (epi) { P.ep = epp->epi; P.eL = epiL; }
    P.mono = mono; P.mono_ran = mono && t->frames > 0;
    P.resident = A.resident;
    P.from_kf = t->from_kf;
    if (mono) {
        P.fkf = epp->epi.fkf;
        P.time.assign(A.min->time_h, A.min->time_h + n_active);
        P.frame_id.assign(A.min->frame_id_h, A.min->frame_id_h + n_active);
        P.localba.assign((size_t)n_active, 0);
        if (A.min->localba_is_on_h) for (int b = 0; b < n_active; b++) P.localba[(size_t)b] = A.min->localba_is_on_h[b] ? 1 : 0;
    }
    // the step proper: the form's blocks staged (and allocated or grown by the first step that needs them), then the enqueue
    auto track = [&]() -> int {
        int r = OV2_OK;
        if (map) {
            r = stage_map(t, n_active, A.wpt_h, A.is3d_h, A.Tcw_h, n_h);  if (r) return r;
            P.has_prior = t->pt.h + t->pl.o_flg;                         // the flags the device sets: same slots as the caller's array
        }
        if (pose) { r = stage_pose(t, n_active, pp, pin, n_h, poseL, A.resident);  if (r) return r; }
        if (epi || mono) {
            r = ensure_epi(t, epi ? &epiL : nullptr);  if (r) return r;
            stage_epi(t, n_active, ein, n_h);
        }
        if (mono) { r = ensure_mono(t);  if (r) return r;  stage_mono(t, P); }
        stage_points(t, n_active, A.kps_xy_h, map ? nullptr : A.prior_xy_h, A.has_prior_h, n_h, A.klt_use_prior);
        if (A.resident) {
            // the frame before the step, as _end reads it on the host: where k_res_stage puts it (zero copy), or from the mirror
            P.kps = (const float *)(t->pt.h + t->pl.o_kps);
            if (t->pt.d) res_fill_host(t, n_active);
        }
        r = preprocess();
        return r ? r : enqueue_klt(t, P.from_kf ? t->kf_store : t->pyr[t->prev()], t->pyr[t->cur], P);
    };
    // the first frame (trackMono returns right after preprocessImage) and a step with nothing to track anywhere only pre-process
    const bool tracked = t->frames > 0 && n_total > 0;
    // mono, not the first frame, no keypoint anywhere: the motion model and the decision run (the reference runs them too)
    auto mono_empty = [&]() -> int {
        int r = stage_map(t, n_active, A.wpt_h, A.is3d_h, nullptr, P.n.data());  if (r) return r;
        r = stage_pose(t, n_active, pp, pin, P.n.data(), poseL);  if (r) return r;
        r = ensure_epi(t, nullptr);  if (r) return r;
        r = ensure_mono(t);  if (r) return r;
        stage_mono(t, P);
        r = preprocess();
        return r ? r : enqueue_mono_empty(t, P);
    };
    rc = tracked ? track() : (P.mono_ran ? mono_empty() : preprocess());
    if (rc != OV2_OK) { t->cur = old_cur; return rc; }
    commit();
    P.tracked = tracked; t->open = CALL_STEP;
    return OV2_OK;
}

// What the one-call forms check before anything is enqueued: the result buffers.  pose / epi: the result arrays of those forms (or
// NULL).  Arguments that track_frame_begin refuses are left to it.
static int check_outputs(const ov2_btracker *t, int n_active, const int *n_h, const float *out_xy_h, const uint8_t *status_h,
                         const ov2_pose_result *pose, const ov2_epifilter_result *epi)
{
    if (!(t && n_active >= 1 && n_active <= t->batch && n_h)) return OV2_OK;
    int n_total = 0;
    for (int b = 0; b < n_active; b++) {
        n_total += n_h[b] > 0 ? n_h[b] : 0;
        if (pose) OV2_REQUIRE(n_h[b] <= 0 || (pose[b].removed && (!epi || epi[b].removed)), OV2_EINVAL, "NULL result buffer (removed)");
        if (epi) OV2_REQUIRE(!epi[b].trace_samples, OV2_EINVAL, "trace_samples must be NULL in a step: ov2_btracker_last_epi_inputs fetches the table");
    }
    OV2_REQUIRE(n_total == 0 || (out_xy_h && status_h), OV2_EINVAL, "NULL point buffer");
    return OV2_OK;
}

extern "C" {

int ov2_btracker_track_frame_begin(ov2_btracker *t, int n_active, const uint8_t *const *img_h, int stride, const float *kps_xy_h,
                                   const float *prior_xy_h, const uint8_t *has_prior_h, const int *n_h, int klt_use_prior)
{
    StepArgs A;
    A.n_active = n_active; A.img_h = img_h; A.stride = stride; A.kps_xy_h = kps_xy_h; A.n_h = n_h; A.klt_use_prior = klt_use_prior;
    A.prior_xy_h = prior_xy_h; A.has_prior_h = has_prior_h;
    return track_frame_begin(t, A);
}

int ov2_btracker_track_frame_map_begin(ov2_btracker *t, int n_active, const uint8_t *const *img_h, int stride, const float *kps_xy_h,
                                       const double *wpt_h, const uint8_t *is3d_h, const double *Tcw_h, const int *n_h, int klt_use_prior)
{
    StepArgs A;
    A.form = STEP_MAP; A.n_active = n_active; A.img_h = img_h; A.stride = stride; A.kps_xy_h = kps_xy_h; A.n_h = n_h; A.klt_use_prior = klt_use_prior;
    A.wpt_h = wpt_h; A.is3d_h = is3d_h; A.Tcw_h = Tcw_h;
    return track_frame_begin(t, A);
}

} // extern "C"

// A query of the last inputs of item b: the slot list and the table's rows (row_bytes each: 16 the pose, 32 the
// filter), from the host lists where the rule re-ran the item, else from the device block (slot_d / tab_d: the item's)
static int last_inputs_fetch(const ov2_btracker *t, const LastInputs &r, size_t b, int *slot_idx, int *samples, const uint8_t *slot_d,
                             const uint8_t *tab_d, size_t row_bytes)
{
    const int n = r.ncur[b], rows = r.rows[b];
    if (r.host[b]) {
        if (slot_idx && n > 0) memcpy(slot_idx, r.slot[b].data(), 4 * (size_t)n);
        if (samples && rows > 0) memcpy(samples, r.samples[b].data(), row_bytes * (size_t)rows);
        return OV2_OK;
    }
    if (!r.chain || (n <= 0 && rows <= 0)) return OV2_OK;
    OV2_HIP_CHECK(hipSetDevice(t->ctx->device));
    if (slot_idx && n > 0 && n <= t->cfg.n_max) OV2_HIP_CHECK(hipMemcpy(slot_idx, slot_d, 4 * (size_t)n, hipMemcpyDeviceToHost));
    if (samples && rows > 0) OV2_HIP_CHECK(hipMemcpy(samples, tab_d, row_bytes * (size_t)rows, hipMemcpyDeviceToHost));
    return OV2_OK;
}

static void pose_store(ov2_pose_result &r, const PoseOut &o)
{
    memcpy(r.Twc, o.Twc, 56);
    r.action = o.action; r.p3p_req_out = o.p3p_req_out; r.n_removed_p3p = o.n_removed_p3p; r.n_outliers_pnp = o.n_outliers_pnp;
    r.ran_p3p = o.ran_p3p; r.p3p_status = o.p3p_status; r.p3p_best_row = o.p3p_best_row; r.p3p_iterations = o.p3p_iterations;
    r.p3p_rows_consumed = o.p3p_rows_consumed; r.p3p_score = o.p3p_score;
    for (int q = 0; q < 2; q++) {
        ov2_pnp_pass &d = r.pass[q];
        d.ran = o.ran[q]; d.iterations = o.iterations[q]; d.num_successful_steps = o.n_success[q]; d.termination = o.termination[q];
        d.initial_cost = o.initial_cost[q]; d.final_cost = o.final_cost[q];
    }
}

// a result as a step leaves it where no chain ran: the caller's pointers kept, their n bytes / values and everything else cleared
static void pose_reset(ov2_pose_result &r, int n, const double *Twc, int req)
{
    uint8_t *removed = r.removed;
    memset(&r, 0, sizeof(r));
    r.removed = removed;
    if (n > 0) memset(removed, 0, (size_t)n);
    memcpy(r.Twc, Twc, 56);
    r.action = OV2_POSE_TOO_FEW; r.p3p_req_out = req != 0;
}

static void epi_reset(ov2_epifilter_result &r, int n)
{
    const ov2_epifilter_result keep = r;
    memset(&r, 0, sizeof(r));
    r.removed = keep.removed; r.pair_cur = keep.pair_cur; r.err = keep.err;
    r.action = OV2_EPIF_TOO_FEW_KPS;
    if (n > 0) memset(r.removed, 0, (size_t)n);
    if (n > 0 && r.err) memset(r.err, 0, 4 * (size_t)n);
}

// The items where the 33 % rule fired (`redo`), after their retry: the pose set from the final status, the step's unpx / bv as the
// retry left them, a table drawn from the new m, and ov2_compute_pose_batch over just those items with do_p3p = p3p_req = 1
// excl (or NULL): one byte per slot, laid out like status_h -- a slot the filter removed is not in the pose set
static int pose_redo(ov2_btracker *t, const std::vector<int> &redo, const uint8_t *status_h, ov2_pose_result *results, const uint8_t *excl)
{
    const ov2_btracker::Pending &P = t->pend;
    const uint8_t *hblk = t->pt.h, *hmap = t->map.h;
    const size_t nm = (size_t)t->cfg.n_max, R = redo.size();
    std::vector<std::vector<double>> unpx(R), wpt(R), bv(R);
    std::vector<std::vector<int>> scale(R);
    std::vector<std::vector<uint8_t>> rm(R);
    std::vector<ov2_pose_problem> pb(R);
    std::vector<ov2_pose_result> rs(R);
    for (size_t k = 0; k < R; k++) {
        const int b = redo[k];
        const size_t o = (size_t)b * nm;
        const int n = P.n[(size_t)b];
        const float *un = (const float *)(hblk + t->pl.o_unpx) + 2 * o;
        const double *bvs = (const double *)(hblk + t->pl.o_bv) + 3 * o, *w = (const double *)(hmap + t->ml.m_w) + 3 * o;
        const uint8_t *d3 = hmap + t->ml.m_3d + o;
        const int *sc = (const int *)(t->pose.h + t->ql.q_sc) + o;
        std::vector<int> &slot = t->lp.slot[(size_t)b];
        slot.clear();
        for (int i = 0; i < n; i++)
            if ((status_h[o + i] & 3) == 1 && d3[i] && !(excl && excl[o + i])) {
                slot.push_back(i);
                unpx[k].push_back((double)un[2 * i]); unpx[k].push_back((double)un[2 * i + 1]);
                for (int c = 0; c < 3; c++) { wpt[k].push_back(w[3 * i + c]); bv[k].push_back(bvs[3 * i + c]); }
                scale[k].push_back(sc[i]);
            }
        const int m = (int)slot.size();
        std::vector<int> &tab = t->lp.samples[(size_t)b];
        tab.clear();
        if (m >= 4 && P.pp.n_rows > 0) {
            tab.resize(4 * (size_t)P.pp.n_rows);
            const int rc = ov2_p3p_draw_samples(P.seed[(size_t)b], m, P.pp.n_rows, tab.data());
            if (rc != OV2_OK) return rc;
        }
        rm[k].assign((size_t)(m > 0 ? m : 1), 0);
        ov2_pose_problem &q = pb[k];
        q.n = m; q.unpx = unpx[k].data(); q.wpt = wpt[k].data(); q.scale = scale[k].data(); q.Twc = P.Twc.data() + 7 * (size_t)b;
        q.bv = bv[k].data(); q.do_p3p = 1; q.p3p_req = 1; q.n_rows = m >= 4 ? P.pp.n_rows : 0; q.samples = tab.empty() ? nullptr : tab.data();
        rs[k].removed = rm[k].data();
        t->lp.ncur[(size_t)b] = t->lp.m[(size_t)b] = m; t->lp.rows[(size_t)b] = q.n_rows; t->lp.host[(size_t)b] = 1;
    }
    const int rc = ov2_compute_pose_batch(t->ctx, &P.pp.pose, (int)R, pb.data(), rs.data());
    if (rc != OV2_OK) return rc;
    for (size_t k = 0; k < R; k++) {
        const int b = redo[k];
        ov2_pose_result &r = results[b];
        pose_reset(r, P.n[(size_t)b], P.Twc.data() + 7 * (size_t)b, 1);
        rs[k].removed = r.removed;                                       // the second run's record, the caller's (cleared) bytes
        r = rs[k];
        const std::vector<int> &slot = t->lp.slot[(size_t)b];
        for (size_t j = 0; j < slot.size(); j++) r.removed[slot[j]] = rm[k][j];
    }
    return OV2_OK;
}

// the record of the chain into the caller's result (its four pointers are the caller's and stay), as ov2_epipolar_filter_batch does
static void epi_store(ov2_epifilter_result &r, const EpifOut &o)
{
    r.action = o.action; r.m = o.m; r.epifrom3dkps = o.epifrom3dkps; r.do_optimize = o.do_optimize; r.nb3dkps = o.nb3dkps;
    r.parallax = o.parallax; r.status = o.status; r.best_row = o.best_row; r.iterations = o.iterations;
    r.rows_consumed = o.rows_consumed; r.score = o.score; r.n_inliers = o.n_inliers; r.n_outliers = o.n_outliers;
    memcpy(r.model, o.model, sizeof o.model); memcpy(r.F, o.F, sizeof o.F); memcpy(r.Twc_model, o.Twc_model, sizeof o.Twc_model);
    r.n_removed_ransac = o.n_removed_ransac; r.n_removed_sampson = o.n_removed_sampson; r.pose_from_model = o.pose_from_model;
}

// rows of the table the filter's search used: it ran (the action is past the two early returns) over at least eight matches
static inline int epi_rows_used(int action, int m, int n_rows) { return action >= OV2_EPIF_NO_MODEL && m >= 8 ? n_rows : 0; }

// The items where the 33 % rule fired, after their retry: the frame from the final status, the step's unpx / bv as the retry left them,
// ov2_epipolar_filter_batch against the keyframes' host copy over just those items, the results to slot space; excl (laid out like
// status_h) gets a byte per slot the filter removed, for the pose set of pose_redo.
static int epi_redo(ov2_btracker *t, const std::vector<int> &redo, const float *out_xy_h, const uint8_t *status_h,
                    ov2_epifilter_result *results, std::vector<uint8_t> &excl)
{
    const ov2_btracker::Pending &P = t->pend;
    const size_t nm = (size_t)t->cfg.n_max, R = redo.size();
    const int n_rows = P.ep.n_rows;
    const int *lmid_h = (const int *)(t->epi.h + t->el.e_lm), *nbkfs_h = (const int *)(t->epi.h + t->el.e_nk);    // as the step staged them
    const unsigned long long *seed_h = (const unsigned long long *)(t->epi.h + t->el.e_sd);
    std::vector<std::vector<int>> lmid(R), pair(R);
    std::vector<std::vector<float>> px(R), unpx(R), err(R);
    std::vector<std::vector<double>> bv(R);
    std::vector<std::vector<uint8_t>> d3(R), rm(R);
    std::vector<ov2_epifilter_item> items(R);
    std::vector<ov2_epifilter_result> rs(R);
    excl.assign(nm * (size_t)P.n_active, 0);
    for (size_t k = 0; k < R; k++) {
        const int b = redo[k];
        const size_t o = (size_t)b * nm;
        const int n = P.n[(size_t)b];
        const float *un = (const float *)(t->pt.h + t->pl.o_unpx) + 2 * o;
        const double *bvs = (const double *)(t->pt.h + t->pl.o_bv) + 3 * o;
        const uint8_t *f3 = t->map.h + t->ml.m_3d + o;
        std::vector<int> &slot = t->le.slot[(size_t)b];
        slot.clear();
        for (int i = 0; i < n; i++)
            if ((status_h[o + i] & 3) == 1) {
                slot.push_back(i);
                lmid[k].push_back(lmid_h[o + i]);
                px[k].push_back(out_xy_h[2 * (o + i)]); px[k].push_back(out_xy_h[2 * (o + i) + 1]);
                unpx[k].push_back(un[2 * i]); unpx[k].push_back(un[2 * i + 1]);
                for (int c = 0; c < 3; c++) bv[k].push_back(bvs[3 * i + c]);
                d3[k].push_back(f3[i]);
            }
        const int nc = (int)slot.size();
        const size_t room = (size_t)(nc > 0 ? nc : 1);
        lmid[k].resize(room); px[k].resize(2 * room); unpx[k].resize(2 * room); bv[k].resize(3 * room); d3[k].resize(room);
        rm[k].assign(room, 0); pair[k].assign(room, 0); err[k].assign(room, 0.f);
        std::vector<int> &tab = t->le.samples[(size_t)b];
        tab.assign(8 * (size_t)(n_rows > 0 ? n_rows : 1), -1);
        const FeKfHdr &h = t->kf_hdr[(size_t)b];
        const KfHost kf = kf_host_item(t, b);
        ov2_epifilter_item &q = items[k];
        memset(&q, 0, sizeof q);
        q.fkf.n_cur = nc; q.fkf.cur_lmid = lmid[k].data(); q.fkf.cur_px = px[k].data(); q.fkf.cur_unpx = unpx[k].data();
        q.fkf.cur_bv = bv[k].data(); q.fkf.cur_is3d = d3[k].data(); q.fkf.cur_Twc = P.Twc.data() + 7 * (size_t)b;
        q.fkf.n_kf = h.n_kf; q.fkf.kf_lmid = kf.lmid; q.fkf.kf_unpx = kf.unpx;
        q.fkf.kf_Tcw = h.kf_Tcw; q.fkf.noccupcells = -1; q.fkf.nb3dkps = -1;
        q.kf_bv = kf.bv; q.kf_Twc = h.kf_Twc; q.nbkfs = nbkfs_h[b]; q.seed = seed_h[b];
        ov2_epifilter_result &r = rs[k];
        memset(&r, 0, sizeof r);
        r.removed = rm[k].data(); r.pair_cur = pair[k].data(); r.err = err[k].data(); r.trace_samples = n_rows > 0 ? tab.data() : nullptr;
    }
    const int rc = ov2_epipolar_filter_batch(t->ctx, &P.ep, (int)R, items.data(), rs.data());
    if (rc != OV2_OK) return rc;
    for (size_t k = 0; k < R; k++) {
        const int b = redo[k];
        const size_t o = (size_t)b * nm;
        const int n = P.n[(size_t)b];
        const std::vector<int> &slot = t->le.slot[(size_t)b];
        ov2_epifilter_result &r = results[b];
        epi_reset(r, n);
        rs[k].removed = r.removed; rs[k].pair_cur = r.pair_cur; rs[k].err = r.err; rs[k].trace_samples = nullptr;
        r = rs[k];                                                       // the second run's record, the caller's (cleared) arrays
        for (size_t j = 0; j < slot.size(); j++) {
            r.removed[slot[j]] = rm[k][j];
            if (r.err) r.err[slot[j]] = err[k][j];
            if (rm[k][j]) excl[o + (size_t)slot[j]] = 1;
        }
        if (r.pair_cur)
            for (int j = 0; j < r.m && j < (int)slot.size(); j++)
                r.pair_cur[j] = (unsigned)pair[k][(size_t)j] < slot.size() ? slot[(size_t)pair[k][(size_t)j]] : -1;
        t->le.ncur[(size_t)b] = (int)slot.size(); t->le.m[(size_t)b] = r.m;
        t->le.rows[(size_t)b] = epi_rows_used(r.action, r.m, n_rows); t->le.host[(size_t)b] = 1;
    }
    return OV2_OK;
}

// both forms of the step's second half.  results != NULL: the step was begun with ov2_btracker_track_frame_pose_begin and its
// poses are wanted; NULL: the tracking half only (a pose the step computed is dropped)
// eres != NULL (with results): the step was begun with ov2_btracker_track_frame_epi_pose_begin and the filter's records are wanted too
// mres != NULL (with results; eres unless the step ran without the filter): the step was begun with ov2_btracker_track_mono_begin;
// redo / excl: the items the rule re-ran and the slots the filter's second run removed, for mono_finish
static int track_frame_end_step(ov2_btracker *t, float *out_xy_h, uint8_t *status_h, int *p3p_req, ov2_pose_result *results,
                                ov2_epifilter_result *eres, const ov2_track_mono_result *mres, std::vector<int> &redo, std::vector<uint8_t> &excl)
{
    OV2_REQUIRE(t, OV2_EINVAL, "NULL tracker");
    ov2_btracker::Pending &P = t->pend;
    OV2_REQUIRE(t->open == CALL_STEP, OV2_EINVAL, "ov2_btracker_track_frame_end without ov2_btracker_track_frame_begin");
    OV2_REQUIRE(!results || P.form >= STEP_POSE, OV2_EINVAL, "ov2_btracker_track_frame_pose_end: the step was not begun with ov2_btracker_track_frame_pose_begin");
    if (results)
        for (int b = 0; b < P.n_active; b++)
            OV2_REQUIRE(P.n[(size_t)b] == 0 || results[b].removed, OV2_EINVAL, "NULL result buffer (removed)");
    OV2_REQUIRE(!eres || P.form == STEP_EPI, OV2_EINVAL, "ov2_btracker_track_frame_epi_pose_end: the step was not begun with ov2_btracker_track_frame_epi_pose_begin");
    OV2_REQUIRE(!results || P.form != STEP_EPI || eres, OV2_EINVAL, "ov2_btracker_track_frame_pose_end: the step was begun with ov2_btracker_track_frame_epi_pose_begin");
    OV2_REQUIRE(!mres || P.mono, OV2_EINVAL, "ov2_btracker_track_mono_end: the step was not begun with ov2_btracker_track_mono_begin");
    OV2_REQUIRE(!(P.mono && results && !mres), OV2_EINVAL, "the step was begun with ov2_btracker_track_mono_begin: finish it with ov2_btracker_track_mono_end");
    if (eres)
        for (int b = 0; b < P.n_active; b++) {
            OV2_REQUIRE(P.n[(size_t)b] == 0 || eres[b].removed, OV2_EINVAL, "NULL result buffer (removed) of the filter");
            OV2_REQUIRE(!eres[b].trace_samples, OV2_EINVAL, "trace_samples must be NULL in a step: ov2_btracker_last_epi_inputs fetches the table");
        }
    t->open = CALL_NONE;
    if (P.mono) {                                                        // the predicted poses: what the pose chain started from
        OV2_HIP_CHECK(hipSetDevice(t->ctx->device));
        if (P.mono_ran) {
            OV2_HIP_CHECK(hipStreamSynchronize(t->ctx->stream));
            memcpy(P.Twc.data(), t->mono.h + t->nl.n_pT, 56 * (size_t)P.n_active);
        } else memcpy(P.Twc.data(), t->res_T.data(), 56 * (size_t)P.n_active);
    }
    if (results) { t->lp.open((size_t)t->batch, P.tracked); t->lp_L = P.L; }
    if (eres) { t->le.open((size_t)t->batch, P.tracked); t->le_L = P.eL; }
    if (!P.tracked)                                                      // first frame / nothing tracked: no chain ran
        for (int b = 0; b < P.n_active; b++) {
            if (results) pose_reset(results[b], P.n[(size_t)b], P.Twc.data() + 7 * (size_t)b, P.req[(size_t)b]);
            if (eres) epi_reset(eres[b], P.n[(size_t)b]);
        }
    const size_t nm = (size_t)t->cfg.n_max;
    ov2_ctx *ctx = t->ctx;
    OV2_HIP_CHECK(hipSetDevice(ctx->device));
    if (p3p_req) for (int b = 0; b < P.n_active; b++) p3p_req[b] = 0;
    if (!P.tracked) {
        if (status_h) for (int b = 0; b < P.n_active; b++) if (P.n[(size_t)b] > 0) memset(status_h + nm * b, 0, (size_t)P.n[(size_t)b]);
        return ov2_ctx_sync(ctx);
    }
    OV2_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    OV2_REQUIRE(out_xy_h && status_h, OV2_EINVAL, "NULL result buffer");
    uint8_t *hblk = t->pt.h;
    const BtPointLayout &pl = t->pl;
    std::vector<int> rule((size_t)P.n_active, 0);
    for (int b = 0; b < P.n_active; b++) {
        const size_t n = (size_t)P.n[(size_t)b], o = nm * (size_t)b;
        if (!n) continue;
        memcpy(out_xy_h + 2 * o, hblk + pl.o_out + 8 * o, 8 * n);
        memcpy(status_h + o, hblk + pl.o_st + o, n);
        // the rule on the item's views; the re-derived unpx / bv go to the item's rows of the point block
        const P3pRuleFrame f = {P.kps + 2 * o, P.has_prior ? P.has_prior + o : nullptr, P.use_prior, (int)n, out_xy_h + 2 * o, status_h + o,
                                (float *)(hblk + pl.o_unpx) + 2 * o, (double *)(hblk + pl.o_bv) + 3 * o};
        int rc;
        if (P.from_kf) {
            const uint8_t *tab = t->kfpx.h + (size_t)b * t->kl.k_item;
            const KfRuleFrame g = {(const int *)(t->epi.h + t->el.e_lm) + o, (const int *)(tab + t->kl.k_lm), (const float *)(tab + t->kl.k_px),
                                   *(const int *)tab, P.has_prior + o, (int)n, f.out_xy, f.status, f.unpx, f.bv};
            rc = ov2_apply_p3p_rule_kf(ctx, t->cfg, t->kf_view[(size_t)b], t->view[t->cur][b], t->has_calib ? &t->calib : nullptr, g, &rule[(size_t)b]);
        } else
            rc = ov2_apply_p3p_rule(ctx, t->cfg, t->view[t->prev()][b], t->view[t->cur][b], t->has_calib ? &t->calib : nullptr, f, &rule[(size_t)b]);
        if (rc != OV2_OK) return rc;
        if (p3p_req) p3p_req[b] = rule[(size_t)b];
        if (t->has_calib) t->last_n[(size_t)b] = (int)n;
        t->last_pn[(size_t)b] = (int)n;
    }
    if (!results) return OV2_OK;
    const uint8_t *hpose = t->pose.h, *hepi = t->epi.h;
    const BtEpiLayout &el = t->el;
    for (int b = 0; b < P.n_active; b++) {
        const size_t n = (size_t)P.n[(size_t)b], o = nm * (size_t)b;
        int ms[2];
        memcpy(ms, hpose + t->ql.q_ms + 8 * (size_t)b, 8);
        t->lp.ncur[(size_t)b] = t->lp.m[(size_t)b] = ms[0]; t->lp.rows[(size_t)b] = ms[1];
        if (n && rule[(size_t)b]) { redo.push_back(b); continue; }
        if (eres) {
            ov2_epifilter_result &r = eres[b];
            EpifOut eo;
            memcpy(&eo, hepi + el.e_out + sizeof(EpifOut) * (size_t)b, sizeof(EpifOut));
            epi_store(r, eo);
            memcpy(&t->le.ncur[(size_t)b], hepi + el.e_nc + 4 * (size_t)b, 4);
            t->le.m[(size_t)b] = eo.m; t->le.rows[(size_t)b] = epi_rows_used(eo.action, eo.m, P.ep.n_rows);
            if (n) {
                memcpy(r.removed, hepi + el.e_rm + o, n);
                if (r.pair_cur && eo.m > 0) memcpy(r.pair_cur, hepi + el.e_pc + 4 * o, 4 * (size_t)(eo.m < (int)n ? eo.m : (int)n));
                if (r.err) memcpy(r.err, hepi + el.e_er + 4 * o, 4 * n);
            }
        }
        PoseOut po;
        memcpy(&po, hpose + t->ql.q_out + sizeof(PoseOut) * (size_t)b, sizeof(PoseOut));
        pose_store(results[b], po);
        if (n) memcpy(results[b].removed, hpose + t->ql.q_rm + o, n);
    }
    if (redo.empty()) return OV2_OK;
    if (eres) { const int rc = epi_redo(t, redo, out_xy_h, status_h, eres, excl);  if (rc != OV2_OK) return rc; }
    return pose_redo(t, redo, status_h, results, eres ? excl.data() : nullptr);
}

// The mono half of _end, behind track_frame_end_step.  mres == NULL: the step is dropped (the plain end call) and the resident pose
// and state go back to what they were.  Else the records of the step; for the items the rule re-ran (redo), updateMotionModel and
// checkNewKfReq again on the second run's pose and frame -- ov2_motion_update_batch from the state BEFORE the step's update,
// ov2_kf_decision_batch on the frame built here by k_mono_pack's rule -- and the corrected pose and state back into the resident block.
static int mono_finish(ov2_btracker *t, const float *out_xy_h, const uint8_t *status_h, const ov2_pose_result *results,
                       ov2_track_mono_result *mres, const std::vector<int> &redo, const std::vector<uint8_t> &excl)
{
    ov2_btracker::Pending &P = t->pend;
    const BtMonoLayout &nl = t->nl;
    const size_t nm = (size_t)t->cfg.n_max;
    if (!mres) return P.mono_ran ? mono_push(t, 0, P.n_active) : OV2_OK;
    const uint8_t *io = t->mono.h;
    for (int b = 0; b < P.n_active; b++) {
        ov2_track_mono_result &r = mres[b];
        memset(&r, 0, sizeof r);
        if (!P.mono_ran) {                                               // the tracker's first frame: trackMono :77
            memcpy(r.Twc_pred, t->res_T.data() + 7 * (size_t)b, 56);
            r.state = t->res_st[(size_t)b];
            r.kf.decision = 1; r.kf.reason = OV2_KF_FIRST_FRAME;
            continue;
        }
        memcpy(r.Twc_pred, io + nl.n_pT + 56 * (size_t)b, 56);
        r.resynced = io[nl.n_rs + (size_t)b];
        memcpy(&r.state, io + nl.n_su + sizeof(ov2_motion_state) * (size_t)b, sizeof(ov2_motion_state));
        const int *o = (const int *)(io + nl.n_dec) + FKF_OUT_INTS * (size_t)b;
        memcpy(&r.kf.parallax, &o[0], 4);
        r.kf.n = o[1]; r.kf.n_distinct = o[2]; r.kf.n_nonfinite = o[3]; r.kf.noccupcells = o[4]; r.kf.nb3dkps = o[5];
        r.kf.n_out_of_grid = o[6]; r.kf.decision = o[7]; r.kf.reason = o[8];
    }
    if (!P.mono_ran) return OV2_OK;
    const size_t R = redo.size();
    if (R) {
        const int *lmid_h = (const int *)(t->epi.h + t->el.e_lm);
        std::vector<std::vector<int>> lmid(R);
        std::vector<std::vector<float>> px(R), unpx(R);
        std::vector<std::vector<double>> bv(R);
        std::vector<std::vector<uint8_t>> d3(R);
        std::vector<ov2_fkf_item> items(R);
        std::vector<ov2_motion_state> sa(R), su(R);
        std::vector<double> Tw(7 * R), tm(R);
        std::vector<ov2_kf_decision_result> dec(R);
        for (size_t k = 0; k < R; k++) {
            const int b = redo[k];
            const size_t o = (size_t)b * nm;
            const ov2_pose_result &pr = results[b];
            const bool reset = pr.action == OV2_POSE_P3P_RESET || pr.action == OV2_POSE_PNP_RESET;          // resetFrame()
            const int n = reset ? 0 : P.n[(size_t)b];
            const float *un = (const float *)(t->pt.h + t->pl.o_unpx) + 2 * o;
            const double *bvs = (const double *)(t->pt.h + t->pl.o_bv) + 3 * o;
            const uint8_t *f3 = t->map.h + t->ml.m_3d + o;
            for (int i = 0; i < n; i++)
                if ((status_h[o + i] & 3) == 1 && !(!excl.empty() && excl[o + i]) && !pr.removed[i]) {
                    lmid[k].push_back(lmid_h[o + i]);
                    px[k].push_back(out_xy_h[2 * (o + i)]); px[k].push_back(out_xy_h[2 * (o + i) + 1]);
                    unpx[k].push_back(un[2 * i]); unpx[k].push_back(un[2 * i + 1]);
                    for (int c = 0; c < 3; c++) bv[k].push_back(bvs[3 * i + c]);
                    d3[k].push_back(f3[i] ? 1 : 0);
                }
            const int nc = (int)lmid[k].size();
            const size_t room = (size_t)(nc > 0 ? nc : 1);
            lmid[k].resize(room); px[k].resize(2 * room); unpx[k].resize(2 * room); bv[k].resize(3 * room); d3[k].resize(room);
            memcpy(&sa[k], io + nl.n_sa + sizeof(ov2_motion_state) * (size_t)b, sizeof(ov2_motion_state));
            memcpy(&Tw[7 * k], pr.Twc, 56);
            tm[k] = P.time[(size_t)b];
            const FeKfHdr &h = t->kf_hdr[(size_t)b];
            const MonoKfInfo &ki = t->res_ki[(size_t)b];
            ov2_fkf_item &q = items[k];
            memset(&q, 0, sizeof q);
            q.n_cur = nc; q.cur_lmid = lmid[k].data(); q.cur_px = px[k].data(); q.cur_unpx = unpx[k].data(); q.cur_bv = bv[k].data();
            q.cur_is3d = d3[k].data(); q.cur_Twc = &Tw[7 * k];
            q.n_kf = h.n_kf; q.kf_lmid = kf_host_item(t, b).lmid; q.kf_unpx = kf_host_item(t, b).unpx; q.kf_Tcw = h.kf_Tcw;
            q.cur_id = P.frame_id[(size_t)b]; q.kf_id = ki.kf_id; q.cur_time = tm[k]; q.kf_time = t->res_kt[(size_t)b];
            q.kf_nb3dkps = ki.kf_nb3dkps; q.localba_is_on = P.localba[(size_t)b]; q.noccupcells = -1; q.nb3dkps = -1;
        }
        int rc = ov2_motion_update_batch(t->ctx, (int)R, sa.data(), Tw.data(), tm.data(), su.data());
        if (rc != OV2_OK) return rc;
        rc = ov2_kf_decision_batch(t->ctx, &P.fkf, (int)R, items.data(), dec.data());
        if (rc != OV2_OK) return rc;
        for (size_t k = 0; k < R; k++) { mres[redo[k]].state = su[k]; mres[redo[k]].kf = dec[k]; }
    }
    for (int b = 0; b < P.n_active; b++) {
        if (t->kf_hdr[(size_t)b].n_kf == 0 || !t->res_ki[(size_t)b].has_info) {                          // :994
            memset(&mres[b].kf, 0, sizeof mres[b].kf);
            mres[b].kf.reason = OV2_KF_NO_KEYFRAME;
        }
        memcpy(t->res_T.data() + 7 * (size_t)b, results[b].Twc, 56);
        t->res_st[(size_t)b] = mres[b].state;
    }
    for (size_t k = 0; k < R; k++) { const int rc = mono_push(t, redo[k], redo[k] + 1);  if (rc != OV2_OK) return rc; }
    return OV2_OK;
}

static int track_frame_end(ov2_btracker *t, float *out_xy_h, uint8_t *status_h, int *p3p_req, ov2_pose_result *results,
                           ov2_epifilter_result *eres, ov2_track_mono_result *mres = nullptr, ov2_resident_step_result *fres = nullptr)
{
    std::vector<int> redo;
    std::vector<uint8_t> excl;
    int rc = track_frame_end_step(t, out_xy_h, status_h, p3p_req, results, eres, mres, redo, excl);
    if (rc != OV2_OK || !t->pend.mono || t->open == CALL_STEP) return rc;
    rc = mono_finish(t, out_xy_h, status_h, results, mres, redo, excl);
    if (rc != OV2_OK || !t->pend.resident || !mres) return rc;
    return res_finish(t, out_xy_h, status_h, results, redo, excl, fres);
}

extern "C" {

int ov2_btracker_track_frame_end(ov2_btracker *t, float *out_xy_h, uint8_t *status_h, int *p3p_req)
{
    return track_frame_end(t, out_xy_h, status_h, p3p_req, nullptr, nullptr);
}

int ov2_btracker_track_frame_pose_begin(ov2_btracker *t, int n_active, const uint8_t *const *img_h, int stride, const float *kps_xy_h,
                                        const double *wpt_h, const uint8_t *is3d_h, const double *Tcw_h, const int *n_h,
                                        int klt_use_prior, const ov2_frame_pose_params *params, const ov2_frame_pose_input *input)
{
    StepArgs A;
    A.form = STEP_POSE; A.n_active = n_active; A.img_h = img_h; A.stride = stride; A.kps_xy_h = kps_xy_h; A.n_h = n_h; A.klt_use_prior = klt_use_prior;
    A.wpt_h = wpt_h; A.is3d_h = is3d_h; A.Tcw_h = Tcw_h; A.pp = params; A.pin = input;
    return track_frame_begin(t, A);
}

int ov2_btracker_track_frame_pose_end(ov2_btracker *t, float *out_xy_h, uint8_t *status_h, int *p3p_req, ov2_pose_result *results)
{
    OV2_REQUIRE(results, OV2_EINVAL, "NULL result array");
    return track_frame_end(t, out_xy_h, status_h, p3p_req, results, nullptr);
}

int ov2_btracker_track_frame_pose(ov2_btracker *t, int n_active, const uint8_t *const *img_h, int stride, const float *kps_xy_h,
                                  const double *wpt_h, const uint8_t *is3d_h, const double *Tcw_h, const int *n_h, int klt_use_prior,
                                  const ov2_frame_pose_params *params, const ov2_frame_pose_input *input,
                                  float *out_xy_h, uint8_t *status_h, int *p3p_req, ov2_pose_result *results)
{
    OV2_REQUIRE(results, OV2_EINVAL, "NULL result array");
    int rc = check_outputs(t, n_active, n_h, out_xy_h, status_h, results, nullptr);
    if (rc == OV2_OK) rc = ov2_btracker_track_frame_pose_begin(t, n_active, img_h, stride, kps_xy_h, wpt_h, is3d_h, Tcw_h, n_h, klt_use_prior, params, input);
    if (rc != OV2_OK) return rc;
    return track_frame_end(t, out_xy_h, status_h, p3p_req, results, nullptr);
}

int ov2_btracker_last_pose_inputs(const ov2_btracker *t, int item, int *m, int *slot_idx, int *samples, int *n_rows_used)
{
    OV2_REQUIRE(t, OV2_EINVAL, "NULL tracker");
    OV2_REQUIRE(item >= 0 && item < t->batch, OV2_EINVAL, "batch item out of range");
    OV2_REQUIRE(t->lp.on, OV2_EINVAL, "ov2_btracker_last_pose_inputs: no pose step has been finished on this tracker");
    const size_t b = (size_t)item;
    if (m) *m = t->lp.m[b];
    if (n_rows_used) *n_rows_used = t->lp.rows[b];
    const PoseLayout &L = t->lp_L;
    const uint8_t *w = t->lp.chain ? t->work.d : nullptr;
    return last_inputs_fetch(t, t->lp, b, slot_idx, samples, w ? w + ov2_frame_pose_slot_offset(L) + 4 * b * (size_t)L.n_max : nullptr,
                             w ? w + L.o_p3 + L.pl.o_sm + 16 * b * (size_t)L.n_rows : nullptr, 16);
}

int ov2_btracker_set_keyframe(ov2_btracker *t, int item, int n_kf, const int *kf_lmid, const float *kf_unpx, const double *kf_bv,
                              const double *kf_Twc)
{
    OV2_REQUIRE(t, OV2_EINVAL, "NULL tracker");
    OV2_REQUIRE(item >= 0 && item < t->batch, OV2_EINVAL, "batch item out of range");
    OV2_REQUIRE(n_kf >= 0, OV2_EINVAL, "negative count (n_kf)");
    OV2_REQUIRE(n_kf <= OV2_FKF_MAX_POINTS, OV2_EINVAL, "more than OV2_FKF_MAX_POINTS (2048) keypoints in the keyframe");
    OV2_REQUIRE(n_kf <= t->cfg.n_max, OV2_EINVAL, "the keyframe carries more keypoints than cfg.n_max slots");
    OV2_REQUIRE(t->cfg.n_max <= OV2_FKF_MAX_POINTS, OV2_EINVAL, "capacity: cfg.n_max exceeds OV2_FKF_MAX_POINTS (2048) keypoints of one frame");
    OV2_REQUIRE(n_kf == 0 || (kf_lmid && kf_unpx), OV2_EINVAL, "NULL array of the keyframe (kf_lmid / kf_unpx)");
    OV2_REQUIRE(n_kf == 0 || (kf_bv && kf_Twc), OV2_EINVAL, "NULL kf_bv / kf_Twc");
    for (int i = 1; i < n_kf; i++) OV2_REQUIRE(kf_lmid[i - 1] < kf_lmid[i], OV2_EINVAL, "kf_lmid unsorted: not strictly ascending");
    FeKfHdr h = FeKfHdr();
    h.n_kf = n_kf;
    if (kf_Twc) {
        for (int c = 0; c < 7; c++) OV2_REQUIRE(std::isfinite(kf_Twc[c]), OV2_EINVAL, "pose not finite (kf_Twc)");
        memcpy(h.kf_Twc, kf_Twc, 56);
        ov2_fe_invert(kf_Twc, h.kf_Tcw);
        for (int c = 0; c < 7; c++) OV2_REQUIRE(std::isfinite(h.kf_Tcw[c]), OV2_EINVAL, "pose not finite (the inverse of kf_Twc)");
    }
    for (size_t i = 0; i < 3 * (size_t)n_kf; i++) OV2_REQUIRE(std::isfinite(kf_bv[i]), OV2_EINVAL, "kf_bv not finite");
    OV2_REQUIRE(!t->open_call(), OV2_EINVAL, "ov2_btracker_set_keyframe between steps only: a step is open");
    const int rc = ensure_epi(t, nullptr);
    if (rc != OV2_OK) return rc;
    const EpifLayout &L0 = t->eL0;
    const size_t o = (size_t)item * (size_t)t->cfg.n_max, n = (size_t)n_kf;
    const KfHost kf = kf_host_item(t, item);
    hipStream_t s = t->ctx->stream;
    if (n) {
        memcpy(kf.lmid, kf_lmid, 4 * n);
        memcpy(kf.unpx, kf_unpx, 8 * n);
        memcpy(kf.bv, kf_bv, 24 * n);
        OV2_HIP_CHECK(hipMemcpyAsync(t->depi + L0.o_kl + 4 * o, kf.lmid, 4 * n, hipMemcpyHostToDevice, s));
        OV2_HIP_CHECK(hipMemcpyAsync(t->depi + L0.o_ku + 8 * o, kf.unpx, 8 * n, hipMemcpyHostToDevice, s));
        OV2_HIP_CHECK(hipMemcpyAsync(t->depi + L0.o_kb + 24 * o, kf.bv, 24 * n, hipMemcpyHostToDevice, s));
    }
    t->kf_hdr[(size_t)item] = h;
    if (!t->res_iskf.empty()) t->res_iskf[(size_t)item] = 0;
    if (!t->from_kf && !t->kf_has_pyr.empty()) t->kf_has_pyr[(size_t)item] = 0;      // a keyframe set with the mode off: the store's is stale
    OV2_HIP_CHECK(hipMemcpyAsync(t->fx.d + sizeof(FeKfHdr) * (size_t)item, &t->kf_hdr[(size_t)item], sizeof(FeKfHdr), hipMemcpyHostToDevice, s));
    OV2_HIP_CHECK(hipStreamSynchronize(s));                              // the host copy may be rewritten by the next call
    return OV2_OK;
}

int ov2_btracker_track_frame_epi_pose_begin(ov2_btracker *t, int n_active, const uint8_t *const *img_h, int stride, const float *kps_xy_h,
                                            const double *wpt_h, const uint8_t *is3d_h, const double *Tcw_h, const int *n_h,
                                            int klt_use_prior, const ov2_frame_epi_pose_params *params,
                                            const ov2_frame_epi_pose_input *input)
{
    StepArgs A;
    A.form = STEP_EPI; A.n_active = n_active; A.img_h = img_h; A.stride = stride; A.kps_xy_h = kps_xy_h; A.n_h = n_h; A.klt_use_prior = klt_use_prior;
    A.wpt_h = wpt_h; A.is3d_h = is3d_h; A.Tcw_h = Tcw_h; A.epp = params; A.ein = input;
    return track_frame_begin(t, A);
}

int ov2_btracker_track_frame_epi_pose_end(ov2_btracker *t, float *out_xy_h, uint8_t *status_h, int *p3p_req,
                                          ov2_epifilter_result *epi_results, ov2_pose_result *pose_results)
{
    OV2_REQUIRE(epi_results && pose_results, OV2_EINVAL, "NULL result array");
    return track_frame_end(t, out_xy_h, status_h, p3p_req, pose_results, epi_results);
}

int ov2_btracker_track_frame_epi_pose(ov2_btracker *t, int n_active, const uint8_t *const *img_h, int stride, const float *kps_xy_h,
                                      const double *wpt_h, const uint8_t *is3d_h, const double *Tcw_h, const int *n_h, int klt_use_prior,
                                      const ov2_frame_epi_pose_params *params, const ov2_frame_epi_pose_input *input,
                                      float *out_xy_h, uint8_t *status_h, int *p3p_req, ov2_epifilter_result *epi_results,
                                      ov2_pose_result *pose_results)
{
    OV2_REQUIRE(epi_results && pose_results, OV2_EINVAL, "NULL result array");
    int rc = check_outputs(t, n_active, n_h, out_xy_h, status_h, pose_results, epi_results);
    if (rc == OV2_OK) rc = ov2_btracker_track_frame_epi_pose_begin(t, n_active, img_h, stride, kps_xy_h, wpt_h, is3d_h, Tcw_h, n_h, klt_use_prior, params, input);
    if (rc != OV2_OK) return rc;
    return track_frame_end(t, out_xy_h, status_h, p3p_req, pose_results, epi_results);
}

int ov2_btracker_set_pose(ov2_btracker *t, int item, const double Twc[7])
{
    int rc = mono_item(t, item, "ov2_btracker_set_pose between steps only: a step is open");
    if (rc != OV2_OK) return rc;
    OV2_REQUIRE(Twc, OV2_EINVAL, "NULL pose");
    for (int c = 0; c < 7; c++) OV2_REQUIRE(std::isfinite(Twc[c]), OV2_EINVAL, "pose not finite");
    memcpy(t->res_T.data() + 7 * (size_t)item, Twc, 56);
    return mono_push(t, item, item + 1);
}

int ov2_btracker_get_pose(ov2_btracker *t, int item, double Twc[7])
{
    int rc = mono_item(t, item, "ov2_btracker_get_pose between steps only: a step is open");
    if (rc != OV2_OK) return rc;
    OV2_REQUIRE(Twc, OV2_EINVAL, "NULL pose");
    memcpy(Twc, t->res_T.data() + 7 * (size_t)item, 56);
    return OV2_OK;
}

int ov2_btracker_reset_motion(ov2_btracker *t, int item)
{
    int rc = mono_item(t, item, "ov2_btracker_reset_motion between steps only: a step is open");
    if (rc != OV2_OK) return rc;
    ov2_motion_state &s = t->res_st[(size_t)item];                      // MotionModel::reset(): prevTwc_ stays
    s.prev_time = -1.;
    for (int c = 0; c < 6; c++) s.log_relT[c] = 0.;
    return mono_push(t, item, item + 1);
}

int ov2_btracker_get_motion(ov2_btracker *t, int item, ov2_motion_state *state)
{
    int rc = mono_item(t, item, "ov2_btracker_get_motion between steps only: a step is open");
    if (rc != OV2_OK) return rc;
    OV2_REQUIRE(state, OV2_EINVAL, "NULL state");
    *state = t->res_st[(size_t)item];
    return OV2_OK;
}

int ov2_btracker_set_keyframe_info(ov2_btracker *t, int item, int kf_id, double kf_time, int kf_nb3dkps)
{
    int rc = mono_item(t, item, "ov2_btracker_set_keyframe_info between steps only: a step is open");
    if (rc != OV2_OK) return rc;
    OV2_REQUIRE(std::isfinite(kf_time), OV2_EINVAL, "kf_time not finite");
    t->res_ki[(size_t)item] = MonoKfInfo{kf_id, kf_nb3dkps, 1, 0};
    t->res_kt[(size_t)item] = kf_time;
    return mono_push(t, item, item + 1);
}

int ov2_btracker_track_mono_begin(ov2_btracker *t, int n_active, const uint8_t *const *img_h, int stride, const float *kps_xy_h,
                                  const double *wpt_h, const uint8_t *is3d_h, const int *n_h, int klt_use_prior,
                                  const ov2_track_mono_params *params, const ov2_track_mono_input *input)
{
    StepArgs A;
    A.form = STEP_MONO; A.n_active = n_active; A.img_h = img_h; A.stride = stride; A.kps_xy_h = kps_xy_h; A.n_h = n_h; A.klt_use_prior = klt_use_prior;
    A.wpt_h = wpt_h; A.is3d_h = is3d_h; A.mp = params; A.min = input;
    return track_frame_begin(t, A);
}

int ov2_btracker_track_mono_end(ov2_btracker *t, float *out_xy_h, uint8_t *status_h, int *p3p_req, ov2_epifilter_result *epi_results,
                                ov2_pose_result *pose_results, ov2_track_mono_result *mono_results)
{
    OV2_REQUIRE(pose_results && mono_results, OV2_EINVAL, "NULL result array");
    OV2_REQUIRE(t, OV2_EINVAL, "NULL tracker");
    OV2_REQUIRE(t->open != CALL_STEP || !t->pend.mono || (t->pend.form == STEP_EPI) == (epi_results != nullptr), OV2_EINVAL,
                "ov2_btracker_track_mono_end: epi_results goes with doepipolar == 1, and only with it");
    return track_frame_end(t, out_xy_h, status_h, p3p_req, pose_results, epi_results, mono_results);
}

int ov2_btracker_track_mono(ov2_btracker *t, int n_active, const uint8_t *const *img_h, int stride, const float *kps_xy_h,
                            const double *wpt_h, const uint8_t *is3d_h, const int *n_h, int klt_use_prior,
                            const ov2_track_mono_params *params, const ov2_track_mono_input *input, float *out_xy_h, uint8_t *status_h,
                            int *p3p_req, ov2_epifilter_result *epi_results, ov2_pose_result *pose_results,
                            ov2_track_mono_result *mono_results)
{
    OV2_REQUIRE(pose_results && mono_results, OV2_EINVAL, "NULL result array");
    OV2_REQUIRE(!params || (params->doepipolar != 0) == (epi_results != nullptr), OV2_EINVAL,
                "ov2_btracker_track_mono: epi_results goes with doepipolar == 1, and only with it");
    int rc = check_outputs(t, n_active, n_h, out_xy_h, status_h, pose_results, epi_results);
    if (rc == OV2_OK) rc = ov2_btracker_track_mono_begin(t, n_active, img_h, stride, kps_xy_h, wpt_h, is3d_h, n_h, klt_use_prior, params, input);
    if (rc != OV2_OK) return rc;
    return track_frame_end(t, out_xy_h, status_h, p3p_req, pose_results, epi_results, mono_results);
}

// ---- the resident frame (f21): the setters, the getter, the map's ops, and the step on it ----
// what the calls around the resident frame share: the item, no open step, the buffers
static int res_entry(ov2_btracker *t, int item0, int n_items, const char *open_msg)
{
    OV2_REQUIRE(t, OV2_EINVAL, "NULL tracker");
    OV2_REQUIRE(n_items >= 1 && item0 >= 0 && item0 <= t->batch - n_items, OV2_EINVAL, "batch item out of range");
    OV2_REQUIRE(!t->open_call(), OV2_EINVAL, open_msg);
    return ensure_res(t);
}

int ov2_btracker_set_frame(ov2_btracker *t, int item, int n, const float *px, const int *lmid, const uint8_t *is3d, const double *wpt)
{
    OV2_REQUIRE(t, OV2_EINVAL, "NULL tracker");
    OV2_REQUIRE(n >= 0 && n <= t->cfg.n_max, OV2_EINVAL, "ov2_btracker_set_frame: n outside [0, cfg.n_max]");
    OV2_REQUIRE(n == 0 || (px && lmid && is3d && wpt), OV2_EINVAL, "ov2_btracker_set_frame: NULL array");
    std::vector<int> ids(lmid, lmid + n);
    std::sort(ids.begin(), ids.end());
    for (int i = 0; i < n; i++) {
        OV2_REQUIRE(std::isfinite(px[2 * i]) && std::isfinite(px[2 * i + 1]), OV2_EINVAL, "ov2_btracker_set_frame: px not finite");
        OV2_REQUIRE(!is3d[i] || (std::isfinite(wpt[3 * i]) && std::isfinite(wpt[3 * i + 1]) && std::isfinite(wpt[3 * i + 2])), OV2_EINVAL,
                    "ov2_btracker_set_frame: wpt not finite on a 3-D slot");
        OV2_REQUIRE(ids[(size_t)i] >= 0 && (i == 0 || ids[(size_t)i - 1] != ids[(size_t)i]), OV2_EINVAL, "ov2_btracker_set_frame: a negative or repeated lmid");
    }
    int rc = res_entry(t, item, 1, "ov2_btracker_set_frame between steps only: a step is open");
    if (rc != OV2_OK) return rc;
    const ResHost f = res_host(t, item, 0);
    t->res_iskf[(size_t)item] = 0;
    *f.n = n;
    if (n) { memcpy(f.px, px, 8 * (size_t)n); memcpy(f.lmid, lmid, 4 * (size_t)n); memcpy(f.wpt, wpt, 24 * (size_t)n); }
    for (int i = 0; i < n; i++) f.is3d[i] = is3d[i] ? 1 : 0;
    rc = res_push_item(t, item, 0, t->ctx->stream);
    if (rc != OV2_OK) return rc;
    OV2_HIP_CHECK(hipStreamSynchronize(t->ctx->stream));
    return OV2_OK;
}

int ov2_btracker_get_frame(ov2_btracker *t, int item, int from_device, int *n, float *px, int *lmid, uint8_t *is3d, double *wpt)
{
    int rc = res_entry(t, item, 1, "ov2_btracker_get_frame between steps only: a step is open");
    if (rc != OV2_OK) return rc;
    const BtResLayout &L = t->rl;
    const uint8_t *p = (const uint8_t *)res_host(t, item, 0).n;
    std::vector<uint8_t> dev;
    if (from_device) {
        dev.resize(L.f_item);
        OV2_HIP_CHECK(hipMemcpyAsync(dev.data(), t->fr.d + (p - t->fr.h), L.f_item, hipMemcpyDeviceToHost, t->ctx->stream));
        OV2_HIP_CHECK(hipStreamSynchronize(t->ctx->stream));
        p = dev.data();
    }
    int m;
    memcpy(&m, p + L.f_n, 4);
    m = m < 0 ? 0 : (m > t->cfg.n_max ? t->cfg.n_max : m);
    if (n) *n = m;
    if (px) memcpy(px, p + L.f_px, 8 * (size_t)m);
    if (lmid) memcpy(lmid, p + L.f_lm, 4 * (size_t)m);
    if (is3d) memcpy(is3d, p + L.f_3d, (size_t)m);
    if (wpt) memcpy(wpt, p + L.f_w, 24 * (size_t)m);
    return OV2_OK;
}

} // extern "C"

// items [b0, b0 + nb): the ops checked, packed into the control block, one copy up, k_res_update, the records down; the mirror
// advanced by the same rule
static int res_update(ov2_btracker *t, int b0, int nb, const int *n_ops_h, const ov2_resident_op *const *ops_h,
                      ov2_resident_update_result *results)
{
    OV2_REQUIRE(t && n_ops_h && ops_h && results, OV2_EINVAL, "ov2_btracker_update_frame: NULL argument");
    OV2_REQUIRE(nb >= 1 && b0 >= 0 && b0 <= t->batch - nb, OV2_EINVAL, "batch item out of range");
    const int nm = t->cfg.n_max;
    size_t total = 0;
    std::vector<int> ids;
    for (int k = 0; k < nb; k++) {
        const int n = n_ops_h[k];
        OV2_REQUIRE(n >= 0 && n <= nm, OV2_EINVAL, "ov2_btracker_update_frame: n_ops outside [0, cfg.n_max]");
        OV2_REQUIRE(n == 0 || ops_h[k], OV2_EINVAL, "ov2_btracker_update_frame: NULL op list");
        ids.clear();
        for (int j = 0; j < n; j++) {
            const ov2_resident_op &q = ops_h[k][j];
            OV2_REQUIRE(q.op == OV2_RES_SET_POINT || q.op == OV2_RES_UNSET_POINT || q.op == OV2_RES_REMOVE, OV2_EINVAL, "ov2_btracker_update_frame: unknown op");
            OV2_REQUIRE(q.op != OV2_RES_SET_POINT || (std::isfinite(q.xyz[0]) && std::isfinite(q.xyz[1]) && std::isfinite(q.xyz[2])), OV2_EINVAL,
                        "ov2_btracker_update_frame: xyz not finite on OV2_RES_SET_POINT");
            ids.push_back(q.lmid);
        }
        std::sort(ids.begin(), ids.end());
        OV2_REQUIRE(std::adjacent_find(ids.begin(), ids.end()) == ids.end(), OV2_EINVAL, "ov2_btracker_update_frame: an lmid repeated within one item's list");
        total += (size_t)n;
    }
    int rc = res_entry(t, b0, nb, "ov2_btracker_update_frame between steps only: a step is open");
    if (rc != OV2_OK) return rc;
    const BtResLayout &L = t->rl;
    const hipStream_t s = t->ctx->stream;
    uint8_t *h = t->ctl.h, *d = t->ctl.d;
    memcpy(h + L.u_sel, t->res_sel.data(), (size_t)t->batch);
    int *nop = (int *)(h + L.u_nop), *off = (int *)(h + L.u_off);
    ov2_resident_op *ops = (ov2_resident_op *)(h + L.u_ops);
    size_t at = 0;
    for (int k = 0; k < nb; k++) {
        nop[b0 + k] = n_ops_h[k]; off[b0 + k] = (int)at;
        if (n_ops_h[k]) memcpy(ops + at, ops_h[k], sizeof(ov2_resident_op) * (size_t)n_ops_h[k]);
        at += (size_t)n_ops_h[k];
    }
    rc = t->ctl.up(s, 0, L.u_ops + sizeof(ov2_resident_op) * total);  if (rc != OV2_OK) return rc;
    ResUpdateArgs a;
    a.f = res_frames(t);
    a.n_ops = (const int *)(d + L.u_nop); a.op_off = (const int *)(d + L.u_off); a.ops = (const ov2_resident_op *)(d + L.u_ops);
    a.rec = (ov2_resident_update_result *)(d + L.u_rec);
    rc = ov2_launch_res_update(s, a, b0, nb, (int)total);
    if (rc != OV2_OK) return rc;
    const size_t ro = L.u_rec + sizeof(ov2_resident_update_result) * (size_t)b0;
    rc = t->ctl.down(s, ro, ro + sizeof(ov2_resident_update_result) * (size_t)nb);  if (rc != OV2_OK) return rc;
    OV2_HIP_CHECK(hipStreamSynchronize(s));
    memcpy(results, h + ro, sizeof(ov2_resident_update_result) * (size_t)nb);
    // the mirror, by the kernel's rule (an id stands once in a frame and once in a list)
    std::vector<std::pair<int, int>> byid;
    for (int k = 0; k < nb; k++) {
        const int b = b0 + k, n_ops = n_ops_h[k];
        byid.clear();
        for (int j = 0; j < n_ops; j++) byid.push_back({ops_h[k][j].lmid, j});
        std::sort(byid.begin(), byid.end());
        const ResHost src = res_host(t, b, 0), dst = res_host(t, b, 1);
        const int n = *src.n;
        int r = 0;
        for (int i = 0; i < n; i++) {
            const auto it = std::lower_bound(byid.begin(), byid.end(), std::make_pair(src.lmid[i], 0));
            const ov2_resident_op *q = it != byid.end() && it->first == src.lmid[i] ? &ops_h[k][it->second] : nullptr;
            if (q && q->op == OV2_RES_REMOVE) continue;
            dst.px[2 * r] = src.px[2 * i]; dst.px[2 * r + 1] = src.px[2 * i + 1];
            dst.lmid[r] = src.lmid[i];
            dst.is3d[r] = q && q->op == OV2_RES_SET_POINT ? 1 : (q && q->op == OV2_RES_UNSET_POINT ? 0 : src.is3d[i]);
            for (int c = 0; c < 3; c++) dst.wpt[3 * r + c] = q && q->op == OV2_RES_SET_POINT ? q->xyz[c] : src.wpt[3 * i + c];
            r++;
        }
        *dst.n = r;
        t->res_sel[(size_t)b] ^= 1;
        if (r != n) t->res_iskf[(size_t)b] = 0;                          // a slot left: the frame is no longer the keyframe's
    }
    return OV2_OK;
}

extern "C" {

int ov2_btracker_update_frame(ov2_btracker *t, int item, int n_ops, const ov2_resident_op *ops, ov2_resident_update_result *result)
{
    return res_update(t, item, 1, &n_ops, &ops, result);
}

int ov2_btracker_update_frame_batch(ov2_btracker *t, int n_active, const int *n_ops_h, const ov2_resident_op *const *ops_h,
                                    ov2_resident_update_result *results)
{
    return res_update(t, 0, n_active, n_ops_h, ops_h, results);
}

int ov2_btracker_track_mono_resident_begin(ov2_btracker *t, int n_active, const uint8_t *const *img_h, int stride, int klt_use_prior,
                                           const ov2_track_mono_params *params, const ov2_track_mono_input *input)
{
    OV2_REQUIRE(t && params && input, OV2_EINVAL, "ov2_btracker_track_mono_resident: NULL tracker / params / input");
    OV2_REQUIRE(!input->step.lmid_h && !input->step.pose.scale_h, OV2_EINVAL,
                "ov2_btracker_track_mono_resident: lmid_h and scale_h must be NULL (the frame is resident, every scale is 0)");
    OV2_REQUIRE(n_active >= 1 && n_active <= t->batch, OV2_EINVAL, "n_active out of range");
    const int rc = res_entry(t, 0, n_active, "ov2_btracker_track_frame_begin: a step or an ov2_btracker_create_keyframe call is open");
    if (rc != OV2_OK) return rc;
    std::vector<int> n((size_t)n_active);
    for (int b = 0; b < n_active; b++) n[(size_t)b] = *res_host(t, b, 0).n;
    StepArgs A;
    A.form = STEP_MONO; A.resident = true; A.n_active = n_active; A.img_h = img_h; A.stride = stride; A.n_h = n.data();
    A.klt_use_prior = klt_use_prior; A.mp = params; A.min = input;
    return track_frame_begin(t, A);
}

int ov2_btracker_track_mono_resident_end(ov2_btracker *t, float *out_xy_h, uint8_t *status_h, int *p3p_req,
                                         ov2_epifilter_result *epi_results, ov2_pose_result *pose_results,
                                         ov2_track_mono_result *mono_results, ov2_resident_step_result *frame_results)
{
    OV2_REQUIRE(pose_results && mono_results, OV2_EINVAL, "NULL result array");
    OV2_REQUIRE(t, OV2_EINVAL, "NULL tracker");
    OV2_REQUIRE(t->open != CALL_STEP || t->pend.resident, OV2_EINVAL,
                "ov2_btracker_track_mono_resident_end: the step was not begun with ov2_btracker_track_mono_resident_begin");
    OV2_REQUIRE(t->open != CALL_STEP || (t->pend.form == STEP_EPI) == (epi_results != nullptr), OV2_EINVAL,
                "ov2_btracker_track_mono_end: epi_results goes with doepipolar == 1, and only with it");
    return track_frame_end(t, out_xy_h, status_h, p3p_req, pose_results, epi_results, mono_results, frame_results);
}

int ov2_btracker_track_mono_resident(ov2_btracker *t, int n_active, const uint8_t *const *img_h, int stride, int klt_use_prior,
                                     const ov2_track_mono_params *params, const ov2_track_mono_input *input, float *out_xy_h,
                                     uint8_t *status_h, int *p3p_req, ov2_epifilter_result *epi_results, ov2_pose_result *pose_results,
                                     ov2_track_mono_result *mono_results, ov2_resident_step_result *frame_results)
{
    OV2_REQUIRE(pose_results && mono_results, OV2_EINVAL, "NULL result array");
    OV2_REQUIRE(!params || (params->doepipolar != 0) == (epi_results != nullptr), OV2_EINVAL,
                "ov2_btracker_track_mono: epi_results goes with doepipolar == 1, and only with it");
    if (t && t->fr.d && n_active >= 1 && n_active <= t->batch && t->open != CALL_STEP) {      // the result buffers, against the mirror's counts
        std::vector<int> n((size_t)n_active);
        for (int b = 0; b < n_active; b++) n[(size_t)b] = *res_host(t, b, 0).n;
        const int rc = check_outputs(t, n_active, n.data(), out_xy_h, status_h, pose_results, epi_results);
        if (rc != OV2_OK) return rc;
    }
    const int rc = ov2_btracker_track_mono_resident_begin(t, n_active, img_h, stride, klt_use_prior, params, input);
    if (rc != OV2_OK) return rc;
    return track_frame_end(t, out_xy_h, status_h, p3p_req, pose_results, epi_results, mono_results, frame_results);
}

int ov2_btracker_last_slot_bytes(const ov2_btracker *t, size_t *h2d)
{
    OV2_REQUIRE(t && h2d, OV2_EINVAL, "NULL argument");
    *h2d = t->slot_bytes;
    return OV2_OK;
}

int ov2_btracker_last_epi_inputs(const ov2_btracker *t, int item, int *n_cur, int *slot_idx, int *m, int *samples, int *n_rows_used)
{
    OV2_REQUIRE(t, OV2_EINVAL, "NULL tracker");
    OV2_REQUIRE(item >= 0 && item < t->batch, OV2_EINVAL, "batch item out of range");
    OV2_REQUIRE(t->le.on, OV2_EINVAL, "ov2_btracker_last_epi_inputs: no epipolar step has been finished on this tracker");
    const size_t b = (size_t)item;
    if (n_cur) *n_cur = t->le.ncur[b];
    if (m) *m = t->le.m[b];
    if (n_rows_used) *n_rows_used = t->le.rows[b];
    const EpifLayout &L = t->le_L;
    const bool dev = t->le.chain;
    return last_inputs_fetch(t, t->le, b, slot_idx, samples, dev ? t->fx.d + t->el.x_slot + 4 * b * (size_t)t->cfg.n_max : nullptr,
                             dev ? t->depi + L.o_sm + 32 * b * (size_t)L.s_max : nullptr, 32);
}

int ov2_btracker_track_frame(ov2_btracker *t, int n_active, const uint8_t *const *img_h, int stride, const float *kps_xy_h,
                             const float *prior_xy_h, const uint8_t *has_prior_h, const int *n_h, int klt_use_prior,
                             float *out_xy_h, uint8_t *status_h, int *p3p_req)
{
    int rc = check_outputs(t, n_active, n_h, out_xy_h, status_h, nullptr, nullptr);
    if (rc == OV2_OK) rc = ov2_btracker_track_frame_begin(t, n_active, img_h, stride, kps_xy_h, prior_xy_h, has_prior_h, n_h, klt_use_prior);
    if (rc != OV2_OK) return rc;
    return ov2_btracker_track_frame_end(t, out_xy_h, status_h, p3p_req);
}

int ov2_btracker_track_frame_map(ov2_btracker *t, int n_active, const uint8_t *const *img_h, int stride, const float *kps_xy_h,
                                 const double *wpt_h, const uint8_t *is3d_h, const double *Tcw_h, const int *n_h, int klt_use_prior,
                                 float *out_xy_h, uint8_t *status_h, int *p3p_req)
{
    int rc = check_outputs(t, n_active, n_h, out_xy_h, status_h, nullptr, nullptr);
    if (rc == OV2_OK) rc = ov2_btracker_track_frame_map_begin(t, n_active, img_h, stride, kps_xy_h, wpt_h, is3d_h, Tcw_h, n_h, klt_use_prior);
    if (rc != OV2_OK) return rc;
    return ov2_btracker_track_frame_end(t, out_xy_h, status_h, p3p_req);
}

int ov2_btracker_last_priors(const ov2_btracker *t, int item, int n, float *prior_xy_h, uint8_t *has_prior_h)
{
    OV2_REQUIRE(t, OV2_EINVAL, "NULL tracker");
    OV2_REQUIRE(item >= 0 && item < t->batch, OV2_EINVAL, "batch item out of range");
    OV2_REQUIRE(n >= 0 && n <= t->last_pn[(size_t)item], OV2_EINVAL, "more keypoints than the last tracking call returned for this item");
    const size_t o = (size_t)item * t->cfg.n_max;
    if (prior_xy_h) memcpy(prior_xy_h, t->pt.h + t->pl.o_pri + 8 * o, 8 * (size_t)n);
    if (has_prior_h) memcpy(has_prior_h, t->pt.h + t->pl.o_flg + o, (size_t)n);
    return OV2_OK;
}

int ov2_btracker_last_keypoints(const ov2_btracker *t, int item, int n, float *unpx_xy_h, double *bv_xyz_h)
{
    OV2_REQUIRE(t && t->has_calib, OV2_EINVAL, "no calibration set on this tracker");
    OV2_REQUIRE(item >= 0 && item < t->batch, OV2_EINVAL, "batch item out of range");
    OV2_REQUIRE(n >= 0 && n <= t->last_n[(size_t)item], OV2_EINVAL, "more keypoints than the last tracking call returned for this item");
    const size_t o = (size_t)item * t->cfg.n_max;
    if (unpx_xy_h) memcpy(unpx_xy_h, t->pt.h + t->pl.o_unpx + 8 * o, 8 * (size_t)n);
    if (bv_xyz_h) memcpy(bv_xyz_h, t->pt.h + t->pl.o_bv + 24 * o, 24 * (size_t)n);
    return OV2_OK;
}

int ov2_btracker_detect_singlescale(ov2_btracker *t, int n_active, int cell, const float *cur_xy_h, const int *ncur_h, const int roi[4],
                                    double *quality_inout, int do_subpix, float *out_xy_h, int out_cap, int *out_n_h)
{
    OV2_REQUIRE(quality_inout != nullptr && roi != nullptr, OV2_EINVAL, "quality_inout / roi == NULL");
    return detect_common(t, 1, n_active, cell, cur_xy_h, ncur_h, roi, quality_inout, nullptr, 0, do_subpix, out_xy_h, out_cap, out_n_h);
}

int ov2_btracker_detect_grid_fast(ov2_btracker *t, int n_active, int cell, const float *cur_xy_h, const int *ncur_h, int *fast_th_inout,
                                  int mask_mode, int do_subpix, float *out_xy_h, int out_cap, int *out_n_h)
{
    OV2_REQUIRE(fast_th_inout != nullptr, OV2_EINVAL, "fast_th_inout == NULL");
    return detect_common(t, 0, n_active, cell, cur_xy_h, ncur_h, nullptr, nullptr, fast_th_inout, mask_mode, do_subpix, out_xy_h, out_cap, out_n_h);
}

int ov2_btracker_detect_gftt(ov2_btracker *t, int n_active, const uint8_t *roi_h, int roi_stride, const ov2_gftt_params *params,
                             const float *cur_xy_h, const int *ncur_h, const int *nbmax_h, int do_subpix,
                             float *out_xy_h, int out_cap, int *out_n_h)
{
    OV2_REQUIRE(params != nullptr && nbmax_h != nullptr, OV2_EINVAL, "params / nbmax_h == NULL");
    OV2_REQUIRE(t && n_active >= 1 && n_active <= t->batch, OV2_EINVAL, "n_active out of range");
    for (int b = 0; b < n_active; b++)                 // the host list has out_cap slots per item, whatever the mirrors hold
        OV2_REQUIRE(out_cap >= (nbmax_h[b] == -1 ? params->nmaxpts : nbmax_h[b]), OV2_EINVAL, "out_cap below nb2detect");
    return detect_common(t, 2, n_active, 0, cur_xy_h, ncur_h, nullptr, nullptr, nullptr, 0, do_subpix, out_xy_h, out_cap, out_n_h,
                         roi_h, roi_stride, params, nbmax_h);
}

int ov2_btracker_describe_brief(ov2_btracker *t, int n_active, const float *xy_h, const int *n_h, int cap, uint8_t *desc_h, uint8_t *valid_h)
{
    OV2_REQUIRE(t && n_h, OV2_EINVAL, "NULL argument");
    OV2_REQUIRE(t->raw_which >= 0, OV2_EINVAL, "describeBRIEF: no current frames (no step yet, or their staging set was uploaded / prepared again)");
    OV2_REQUIRE(n_active >= 1 && n_active <= t->raw_n, OV2_EINVAL, "n_active exceeds the items of the current step");
    const int which = t->raw_which;
    const int rc = ov2_brief_run_h(t->ctx, nullptr, t->dimg[which], t->cfg.w, t->cfg.h, t->img_pitch, t->img_bytes, n_active, xy_h, n_h, 0, cap,
                                   desc_h, valid_h);
    if (rc != OV2_OK) return rc;
    // a later upload of this set on the copy stream orders itself after the reads (the call has synchronised: this costs nothing)
    OV2_HIP_CHECK(hipEventRecord(t->used_ev[which], t->ctx->stream));
    return OV2_OK;
}

int ov2_btracker_lckf_prepare(ov2_btracker *t, int n_active, const ov2_lckf_params *params, const float *excl_xy_h, const int *n_excl_h,
                              int excl_cap, ov2_lckf_result *results)
{
    OV2_REQUIRE(t && n_excl_h && results, OV2_EINVAL, "NULL argument");
    OV2_REQUIRE(t->raw_which >= 0, OV2_EINVAL, "keyframe preparation: no current frames (no step yet, or their staging set was uploaded / prepared again)");
    OV2_REQUIRE(n_active >= 1 && n_active <= t->raw_n, OV2_EINVAL, "n_active exceeds the items of the current step");
    const int which = t->raw_which;
    const int rc = ov2_lckf_run_h(t->ctx, nullptr, t->dimg[which], t->cfg.w, t->cfg.h, t->img_pitch, t->img_bytes, n_active, params, excl_xy_h,
                                  n_excl_h, excl_cap, results);
    if (rc != OV2_OK) return rc;
    // a later upload of this set on the copy stream orders itself after the reads (the call has synchronised: this costs nothing)
    OV2_HIP_CHECK(hipEventRecord(t->used_ev[which], t->ctx->stream));
    return OV2_OK;
}

const ov2_pyr *ov2_btracker_cur_pyr(const ov2_btracker *t) { return t ? t->pyr[t->cur] : nullptr; }
const ov2_pyr *ov2_btracker_prev_pyr(const ov2_btracker *t) { return t ? t->pyr[t->prev()] : nullptr; }
int ov2_btracker_pyramid_sets(const ov2_btracker *t) { return t ? BT_SETS : 0; }
const ov2_pyr *ov2_btracker_cur_item(const ov2_btracker *t, int item) { return t && item >= 0 && item < t->batch ? t->view[t->cur][(size_t)item] : nullptr; }
const ov2_pyr *ov2_btracker_prev_item(const ov2_btracker *t, int item) { return t && item >= 0 && item < t->batch ? t->view[t->prev()][(size_t)item] : nullptr; }

} // extern "C"
