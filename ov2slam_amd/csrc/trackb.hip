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
#include "common.hpp"
#include "keypoint_dev.hpp"
#include "pose_dev.hpp"
#include "frameepi_dev.hpp"
#include <cmath>
#include <deque>
#include <new>
#include <vector>

int ov2_launch_compute_keypoints(hipStream_t s, const KpCalib &c, const float *px_d, int n_max, const int *n_dev, float *unpx_d, double *bv_d, int items = 1);
// priors.hip: k_prior_frame on device arrays with n_max point slots per item
int ov2_launch_prior_frame(hipStream_t s, const KpCalib &c, double img_w, double img_h, int use_prior, const void *items_d,
                           const double *Tcw_d, const float *px_d, const uint8_t *is3d_d, const double *wpt_d, float *prior_d,
                           uint8_t *has_prior_d, int n_max, int n_items);

// framepose.hip: the pose set, computePose's chain and the removal bytes in slot space, behind k_compute_keypoints
int ov2_launch_frame_pose(hipStream_t s, const ov2_pose_params *params, const PoseLayout &L, int n_active, bool search,
                          const int *n_d, const uint8_t *status_d, const float *unpx_d, const double *bv_d, const double *wpt_d,
                          const uint8_t *is3d_d, const double *Twc_d, const int *scale_d, const uint8_t *flags_d,
                          const unsigned long long *seed_d, uint8_t *work, PoseOut *out_d, int *ms_d, uint8_t *removed_slot_d,
                          ov2_fp_hook hook = nullptr, void *hook_arg = nullptr);
size_t ov2_frame_pose_work_bytes(const PoseLayout &L);
size_t ov2_frame_pose_slot_offset(const PoseLayout &L);

#define BT_SETS 8       // pyramid sets in rotation: cur, prev, the one being prepared for the next frame, five of slack for the mapper
                        // context (a keyframe's pyramids outlive it by BT_SETS - 1 steps: the keyframe period of the shipped parameter files)
#define BT_IMG_SETS 3   // staging sets: frame f (read by its pre-processing), f + 1 (arriving), f + 2 (being filled by the host)

struct ov2_btracker {
    ov2_ctx *ctx = nullptr;
    ov2_tracker_config cfg;
    int batch = 0;
    // pyramid sets in rotation (cur_pyr_, prev_pyr_, ...): a keyframe's pyramids stay valid for BT_SETS - 1 more steps (BT_SETS - 2
    // when the next frame is prepared ahead), so the mapper contexts that stereo-match it rarely hold the SLAM thread up (with two
    // sets 12 % of the lock-step wall clock was that wait)
    ov2_pyr *pyr[BT_SETS] = {};
    std::vector<ov2_pyr *> view[BT_SETS];    // batch-1 aliases of the items (stereo matching, the p3p retry, single-item detection)
    int cur = 0;                       // index of cur_pyr_ (= (frames - 1) % BT_SETS); prev_pyr_ = pyr[(cur + BT_SETS - 1) % BT_SETS]
    int prev() const { return (cur + BT_SETS - 1) % BT_SETS; }
    long frames = 0;
    // frames: pinned staging sets + their device mirrors; a copy stream for uploads and a stream for pre-processing started ahead
    uint8_t *himg[BT_IMG_SETS] = {nullptr, nullptr, nullptr}, *dimg[BT_IMG_SETS] = {nullptr, nullptr, nullptr};
    size_t img_pitch = 0, img_bytes = 0;          // per item (img_bytes a multiple of 256)
    // ov2_btracker_set_rectification: the uploads of set `which` go to draw[which]; the pre-processing of the set starts with k_remap
    // draw[which] -> dimg[which], so dimg holds the RECTIFIED frames.  used_ev[which] is recorded behind that pre-processing: it covers
    // the remap's reads of draw[which] as it covers the reads of dimg[which]
    const ov2_rectmap *rect = nullptr;
    uint8_t *draw[BT_IMG_SETS] = {nullptr, nullptr, nullptr};      // allocated by the first ov2_btracker_set_rectification
    uint8_t *upload_dst(int which) const { return rect ? draw[which] : dimg[which]; }
    hipStream_t cs = nullptr, ps = nullptr;
    ov2_ctx side;                                 // what the launchers of clahe.hip / pyramid.hip see when they enqueue on `ps`
    uint8_t *lut = nullptr;                       // CLAHE tables of a step (the context's scratch is busy with the detector on the main stream)
    hipEvent_t up_ev[BT_IMG_SETS] = {nullptr, nullptr, nullptr};     // set `which` has arrived in dimg[which] (copy stream)
    hipEvent_t used_ev[BT_IMG_SETS] = {nullptr, nullptr, nullptr};   // the kernels that read dimg[which] are done (main or prep stream)
    int up_n[BT_IMG_SETS] = {0, 0, 0};            // items covered by the pending upload of the set (0: none pending)
    // Frame k lives in pyramid set k % BT_SETS.  pre_count = frames whose preprocessImage has been enqueued (ahead or in order);
    // frames prepared ahead wait in prepq (at most two: the one about to be tracked and the one after it)
    struct Prep { int which, n, set; };
    std::deque<Prep> prepq;
    long pre_count = 0;
    // keypoint block: pinned + mapped (the kernels read / write it through its device alias) or mirrored on the device
    uint8_t *hblk = nullptr, *dblk = nullptr, *kblk = nullptr;
    bool zero_copy = false;
    size_t o_n = 0, o_kps = 0, o_pri = 0, o_flg = 0, in_bytes = 0, o_out = 0, o_st = 0, o_unpx = 0, o_bv = 0, blk_bytes = 0;
    bool has_calib = false;
    KpCalib calib;
    std::vector<int> last_n;           // per item: keypoints of the last track_frame (0 before / after a call that tracked nothing)
    std::vector<int> last_pn;          // the same whether or not a calibration is set (ov2_btracker_last_priors)
    // ov2_btracker_track_frame_map: the map side of a step -- [items 16 B][Tcw 56 B] per item, [wpt 24][is3d 1] per slot --, allocated
    // by the first such step; pinned + mapped or mirrored on the device like the keypoint block
    uint8_t *hmap = nullptr, *dmap = nullptr, *kmap = nullptr;
    size_t m_it = 0, m_T = 0, m_w = 0, m_3d = 0, map_bytes = 0;
    // ov2_btracker_track_frame_pose: the pose side of a step, allocated by the first such step.  hpose, pinned + mapped or mirrored
    // like the keypoint block: [Twc 56][seed 8][flags 1] per item and [scale 4] per slot go up; [PoseOut 168][m, rows 8] per item and
    // [removed 1] per slot come down.  dwork: the chain's block at capacity and the pack's lists (device only; not the context's
    // scratch, which other calls use on the same stream)
    uint8_t *hpose = nullptr, *dpose = nullptr, *kpose = nullptr, *dwork = nullptr;
    size_t q_T = 0, q_seed = 0, q_fl = 0, q_sc = 0, q_in = 0, q_out = 0, q_ms = 0, q_rm = 0, pose_bytes = 0, work_bytes = 0;
    // ov2_btracker_last_pose_inputs: the layout of the last finished pose step; per item m and rows; for an item the rule re-ran, the
    // slot list and the table of the second run (the device block still holds those of the first)
    bool lp_on = false, lp_chain = false;
    PoseLayout lp_L;
    std::vector<int> lp_m, lp_rows;
    std::vector<std::vector<int>> lp_slot, lp_samples;
    std::vector<uint8_t> lp_host;
    // ov2_btracker_track_frame_epi_pose / ov2_btracker_set_keyframe: the epipolar side, allocated by the first of either.
    //   depi   the filter's block (EpifLayout at capacity: batch x n_max slots, batch x n_rows rows; device only).  Its inputs
    //          [0, o_up) do not depend on n_rows, so the resident keyframe arrays stay where they are when a step asks for more rows
    //          and the block is grown (they are then copied again from kf_host).
    //   dfx    [FeKfHdr 120 per item][slot 4][rank 4 per slot] (device only)
    //   hepi   pinned + mapped or mirrored like the keypoint block: [lmid 4 per slot][nbkfs 4][seed 8 per item] go up;
    //          [EpifOut 304][n_cur 4 per item][removed 1][err 4][pair 4 per slot] come down
    uint8_t *depi = nullptr, *dfx = nullptr, *hepi = nullptr, *depi_io = nullptr, *kepi = nullptr;
    size_t depi_bytes = 0, x_slot = 0, x_rank = 0, e_lm = 0, e_nk = 0, e_sd = 0, e_in = 0, e_out = 0, e_nc = 0, e_rm = 0, e_er = 0, e_pc = 0,
           epi_bytes = 0;
    EpifLayout eL0;                                   // the layout with no rows: where the keyframe arrays lie
    std::vector<uint8_t> kf_host;                     // host copy of the block's [o_kl, o_up)
    std::vector<FeKfHdr> kf_hdr;
    FeStep fe;                                        // the arguments of the step being enqueued
    // ov2_btracker_last_epi_inputs: as lp_* above
    bool le_on = false, le_chain = false;
    EpifLayout le_L;
    std::vector<int> le_ncur, le_m, le_rows;
    std::vector<std::vector<int>> le_slot, le_samples;
    std::vector<uint8_t> le_host;
    // keyframe detection: device mirrors of the items' current keypoints and of the detector's output, pinned staging
    uint8_t *d_det = nullptr, *h_det = nullptr; size_t det_in_bytes = 0;
    float *d_out = nullptr; uint8_t *h_out = nullptr; int out_cap = 0;
    uint8_t *d_roi = nullptr;                     // detectGFTT: device copy of the caller's roi mask (w x h, allocated with the first one)
    // a step between ov2_btracker_track_frame_begin and _end: what _end needs to finish it
    struct Pending { bool on = false, tracked = false; int n_active = 0, use_prior = 0; const float *kps = nullptr; const uint8_t *has_prior = nullptr; std::vector<int> n;
                     // a pose step (ov2_btracker_track_frame_pose_begin): its settings and the per-item inputs _end needs again
                     bool pose = false; ov2_frame_pose_params pp; PoseLayout L; std::vector<double> Twc; std::vector<uint8_t> req;
                     std::vector<unsigned long long> seed;
                     // an epipolar + pose step (ov2_btracker_track_frame_epi_pose_begin): the filter's settings (its per-item inputs
                     // stay in hepi, which the device only reads)
                     bool epi = false; ov2_epifilter_params ep; EpifLayout eL; } pend;
    // the raw frames of the current step: items [0, raw_n) of dimg[raw_which], until that set is uploaded / prepared again (describeBRIEF)
    int raw_which = -1, raw_n = 0;
};

static inline size_t up16(size_t v) { return (v + 15) & ~(size_t)15; }
static inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

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
    if (t->hblk) (void)hipHostFree(t->hblk);
    if (t->dblk) (void)hipFree(t->dblk);
    if (t->hmap) (void)hipHostFree(t->hmap);
    if (t->dmap) (void)hipFree(t->dmap);
    if (t->hpose) (void)hipHostFree(t->hpose);
    if (t->dpose) (void)hipFree(t->dpose);
    if (t->dwork) (void)hipFree(t->dwork);
    if (t->depi) (void)hipFree(t->depi);
    if (t->dfx) (void)hipFree(t->dfx);
    if (t->hepi) (void)hipHostFree(t->hepi);
    if (t->depi_io) (void)hipFree(t->depi_io);
    if (t->h_det) (void)hipHostFree(t->h_det);
    if (t->d_det) (void)hipFree(t->d_det);
    if (t->h_out) (void)hipHostFree(t->h_out);
    if (t->d_out) (void)hipFree(t->d_out);
    if (t->d_roi) (void)hipFree(t->d_roi);
    delete t;
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

// kltTracking of items [0, n): keypoint block in, the fused LK launch, computeKeypoint, result block out
// map_use_prior >= 0 (ov2_btracker_track_frame_map): k_prior_frame fills the prior and flag slots from the map side first
// pose (ov2_btracker_track_frame_pose): the pose set, computePose's chain and the removal bytes follow k_compute_keypoints
static int enqueue_klt(ov2_btracker *t, const ov2_pyr *prev, const ov2_pyr *cur, int n, int map_use_prior = -1,
                       const ov2_btracker::Pending *pose = nullptr)
{
    ov2_ctx *ctx = t->ctx;
    const ov2_tracker_config &c = t->cfg;
    if (!t->zero_copy) OV2_HIP_CHECK(hipMemcpyAsync(t->dblk, t->hblk, t->in_bytes, hipMemcpyHostToDevice, ctx->stream));
    uint8_t *k = t->kblk;
    if (map_use_prior >= 0) {
        if (!t->zero_copy) OV2_HIP_CHECK(hipMemcpyAsync(t->dmap, t->hmap, t->map_bytes, hipMemcpyHostToDevice, ctx->stream));
        const uint8_t *m = t->kmap;
        const int rcp = ov2_launch_prior_frame(ctx->stream, t->calib, (double)c.w, (double)c.h, map_use_prior, m + t->m_it,
                                               (const double *)(m + t->m_T), (const float *)(k + t->o_kps), m + t->m_3d,
                                               (const double *)(m + t->m_w), (float *)(k + t->o_pri), k + t->o_flg, c.n_max, n);
        if (rcp != OV2_OK) return rcp;
    }
    int rc = ov2_launch_track_klt(ctx->stream, prev, cur, c.win, c.prior_pyr_lvl, c.nklt_pyr_lvl, c.max_iter, c.eps, c.err_th, c.fb_dist,
                                  c.n_max, (const int *)(k + t->o_n), (const float *)(k + t->o_kps), (const float *)(k + t->o_pri),
                                  k + t->o_flg, (float *)(k + t->o_out), k + t->o_st, nullptr, nullptr, 0.f, ctx->track_impl, n, ctx->lk_acc);
    if (rc != OV2_OK) return rc;
    if (t->has_calib) {
        rc = ov2_launch_compute_keypoints(ctx->stream, t->calib, (const float *)(k + t->o_out), c.n_max, (const int *)(k + t->o_n),
                                          (float *)(k + t->o_unpx), (double *)(k + t->o_bv), n);
        if (rc != OV2_OK) return rc;
    }
    if (pose) {
        if (!t->zero_copy) OV2_HIP_CHECK(hipMemcpyAsync(t->dpose, t->hpose, t->q_in, hipMemcpyHostToDevice, ctx->stream));
        uint8_t *q = t->kpose;
        const uint8_t *m = t->kmap;
        bool search = pose->pp.dop3p != 0;
        for (int b = 0; b < n; b++) search = search || pose->req[(size_t)b];
        ov2_fp_hook hook = nullptr;
        if (pose->epi) {                                                // the filter between the select and the pack (frameepi.hip)
            if (!t->zero_copy) OV2_HIP_CHECK(hipMemcpyAsync(t->depi_io, t->hepi, t->e_in, hipMemcpyHostToDevice, ctx->stream));
            uint8_t *e = t->kepi, *d = t->depi;
            const EpifLayout &EL = pose->eL;
            FeStep &fe = t->fe;
            FeArgs &a = fe.a;
            a.n_dev = (const int *)(k + t->o_n); a.status = k + t->o_st; a.is3d = m + t->m_3d;
            a.unpx = (const float2 *)(k + t->o_unpx); a.bv = (const double *)(k + t->o_bv);
            a.lmid = (const int *)(e + t->e_lm); a.nbkfs = (const int *)(e + t->e_nk); a.seed = (const unsigned long long *)(e + t->e_sd);
            a.Twc = (const double *)(q + t->q_T); a.hdr = (const FeKfHdr *)t->dfx;
            a.items = (EpifItem *)(d + EL.o_it); a.c_lmid = (int *)(d + EL.o_lm); a.c_unpx = (float2 *)(d + EL.o_un);
            a.c_bv = (double *)(d + EL.o_bv); a.c_is3d = d + EL.o_3d;
            a.slot = (int *)(t->dfx + t->x_slot); a.rank = (int *)(t->dfx + t->x_rank);
            a.out = (const EpifOut *)(d + EL.o_out); a.removed = d + EL.o_rm; a.err = (const float *)(d + EL.o_er);
            a.pair_cur = (const int *)(d + EL.o_pc);
            a.sel = nullptr;
            a.out_io = (EpifOut *)(e + t->e_out); a.ncur_io = (int *)(e + t->e_nc); a.removed_io = e + t->e_rm;
            a.err_io = (float *)(e + t->e_er); a.pair_io = (int *)(e + t->e_pc);
            a.n_max = c.n_max; a.n_rows = pose->ep.n_rows;
            fe.params = &pose->ep; fe.L = EL; fe.block = d; fe.n_active = n;
            hook = ov2_frame_epi_hook;
        }
        rc = ov2_launch_frame_pose(ctx->stream, &pose->pp.pose, pose->L, n, search, (const int *)(k + t->o_n), k + t->o_st,
                                   (const float *)(k + t->o_unpx), (const double *)(k + t->o_bv), (const double *)(m + t->m_w), m + t->m_3d,
                                   (const double *)(q + t->q_T), (const int *)(q + t->q_sc), q + t->q_fl,
                                   (const unsigned long long *)(q + t->q_seed), t->dwork, (PoseOut *)(q + t->q_out), (int *)(q + t->q_ms),
                                   q + t->q_rm, hook, &t->fe);
        if (rc != OV2_OK) return rc;
        if (!t->zero_copy)
            OV2_HIP_CHECK(hipMemcpyAsync(t->hpose + t->q_out, t->dpose + t->q_out, t->pose_bytes - t->q_out, hipMemcpyDeviceToHost, ctx->stream));
        if (!t->zero_copy && pose->epi)
            OV2_HIP_CHECK(hipMemcpyAsync(t->hepi + t->e_out, t->depi_io + t->e_out, t->epi_bytes - t->e_out, hipMemcpyDeviceToHost, ctx->stream));
    }
    if (!t->zero_copy)
        OV2_HIP_CHECK(hipMemcpyAsync(t->hblk + t->o_out, t->dblk + t->o_out, t->blk_bytes - t->o_out, hipMemcpyDeviceToHost, ctx->stream));
    if (!t->zero_copy && map_use_prior >= 0)                            // the priors and flags the device set come back with the results
        OV2_HIP_CHECK(hipMemcpyAsync(t->hblk + t->o_pri, t->dblk + t->o_pri, t->in_bytes - t->o_pri, hipMemcpyDeviceToHost, ctx->stream));
    return OV2_OK;
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
    if (!t->hmap) {
        const size_t slots = nm * (size_t)t->batch;
        t->m_it = 0; t->m_T = up256(16 * (size_t)t->batch); t->m_w = up256(t->m_T + 56 * (size_t)t->batch); t->m_3d = up256(t->m_w + 24 * slots);
        t->map_bytes = up256(t->m_3d + slots);
        uint8_t *h = nullptr, *d = nullptr;
        hipError_t e = hipHostMalloc((void **)&h, t->map_bytes, hipHostMallocMapped);
        if (e == hipSuccess && !t->zero_copy) e = hipMalloc((void **)&d, t->map_bytes);
        void *alias = d;
        if (e == hipSuccess && t->zero_copy) e = hipHostGetDevicePointer(&alias, h, 0);
        if (e != hipSuccess || !alias) {
            if (h) (void)hipHostFree(h);
            if (d) (void)hipFree(d);
            (void)hipGetLastError();
            ov2_set_error("ov2_btracker_track_frame_map: %s", hipGetErrorString(e));
            return OV2_ENOMEM;
        }
        memset(h, 0, t->map_bytes);
        t->hmap = h; t->dmap = d; t->kmap = (uint8_t *)alias;
    }
    int *it = (int *)(t->hmap + t->m_it);
    for (int b = 0; b < t->batch; b++) {
        it[4 * b] = (int)((size_t)b * nm); it[4 * b + 1] = b < n_active ? n_h[b] : 0; it[4 * b + 2] = it[4 * b + 3] = 0;
    }
    memcpy(t->hmap + t->m_T, Tcw, 56 * (size_t)n_active);
    for (int b = 0; b < n_active; b++) {
        const size_t n = (size_t)n_h[b], o = (size_t)b * nm;
        if (!n) continue;
        memcpy(t->hmap + t->m_w + 24 * o, wpt + 3 * o, 24 * n);
        memcpy(t->hmap + t->m_3d + o, is3d + o, n);
    }
    return OV2_OK;
}

// what a pose step refuses beyond the map form's checks (n_active and the counts are known to be in range); *L: the chain's layout
static int check_pose(const ov2_btracker *t, int n_active, const double *wpt, const uint8_t *is3d, const int *n_h,
                      const ov2_frame_pose_params *pp, const ov2_frame_pose_input *in, PoseLayout *L)
{
    OV2_REQUIRE(pp && in, OV2_EINVAL, "ov2_btracker_track_frame_pose: NULL params / input");
    OV2_REQUIRE(in->Twc_h && in->p3p_req_h && in->seed_h, OV2_EINVAL, "ov2_btracker_track_frame_pose: NULL Twc_h / p3p_req_h / seed_h");
    int rc = pose_check_params(&pp->pose);  if (rc) return rc;
    OV2_REQUIRE(pp->n_rows >= 0, OV2_EINVAL, "negative count (n_rows)");
    OV2_REQUIRE(pp->n_rows <= OV2_P3P_MAX_ROWS, OV2_EINVAL, "capacity: more than 4096 sample rows in one problem");
    OV2_REQUIRE(t->cfg.n_max <= OV2_P3P_MAX_POINTS, OV2_EINVAL, "capacity: cfg.n_max exceeds the 2048 points of one pose problem");
    rc = pose_layout(t->batch, t->cfg.n_max, pp->n_rows, L);  if (rc) return rc;
    const size_t nm = (size_t)t->cfg.n_max;
    for (int b = 0; b < n_active; b++) {
        for (int c = 0; c < 7; c++) OV2_REQUIRE(std::isfinite(in->Twc_h[7 * (size_t)b + c]), OV2_EINVAL, "Twc not finite");
        const size_t n = (size_t)(n_h ? n_h[b] : 0), o = (size_t)b * nm;
        for (size_t i = 0; i < n; i++) {
            if (in->scale_h) OV2_REQUIRE(in->scale_h[o + i] >= -60 && in->scale_h[o + i] <= 60, OV2_EINVAL, "|scale| > 60");
            if (is3d && wpt && is3d[o + i]) {
                const double *w = wpt + 3 * (o + i);
                OV2_REQUIRE(std::isfinite(w[0]) && std::isfinite(w[1]) && std::isfinite(w[2]), OV2_EINVAL, "wpt not finite on a 3-D slot");
            }
        }
    }
    return OV2_OK;
}

// the pose inputs of a step into hpose (the pose buffers are allocated here by the first pose step, and grown when a step asks for
// more sample rows than any before it)
static int stage_pose(ov2_btracker *t, int n_active, const ov2_frame_pose_params *pp, const ov2_frame_pose_input *in, const int *n_h,
                      const PoseLayout &L)
{
    const size_t nm = (size_t)t->cfg.n_max, B = (size_t)t->batch, slots = nm * B;
    if (!t->hpose) {
        t->q_T = 0; t->q_seed = up256(56 * B); t->q_fl = up256(t->q_seed + 8 * B); t->q_sc = up256(t->q_fl + B); t->q_in = up256(t->q_sc + 4 * slots);
        t->q_out = t->q_in; t->q_ms = up256(t->q_out + sizeof(PoseOut) * B); t->q_rm = up256(t->q_ms + 8 * B); t->pose_bytes = up256(t->q_rm + slots);
        uint8_t *h = nullptr, *d = nullptr;
        hipError_t e = hipHostMalloc((void **)&h, t->pose_bytes, hipHostMallocMapped);
        if (e == hipSuccess && !t->zero_copy) e = hipMalloc((void **)&d, t->pose_bytes);
        void *alias = d;
        if (e == hipSuccess && t->zero_copy) e = hipHostGetDevicePointer(&alias, h, 0);
        if (e != hipSuccess || !alias) {
            if (h) (void)hipHostFree(h);
            if (d) (void)hipFree(d);
            (void)hipGetLastError();
            ov2_set_error("ov2_btracker_track_frame_pose: %s", hipGetErrorString(e));
            return OV2_ENOMEM;
        }
        memset(h, 0, t->pose_bytes);
        t->hpose = h; t->dpose = d; t->kpose = (uint8_t *)alias;
    }
    const size_t need = ov2_frame_pose_work_bytes(L);
    if (need > t->work_bytes) {
        OV2_HIP_CHECK(hipStreamSynchronize(t->ctx->stream));              // (the previous step's chain has long finished: _end waited for it)
        if (t->dwork) (void)hipFree(t->dwork);
        t->dwork = nullptr; t->work_bytes = 0; t->lp_on = false;         // the lists of the last step go with the block
        const hipError_t e = hipMalloc((void **)&t->dwork, need);
        if (e != hipSuccess) { (void)hipGetLastError(); ov2_set_error("ov2_btracker_track_frame_pose: %s", hipGetErrorString(e)); return OV2_ENOMEM; }
        t->work_bytes = need;
    }
    memcpy(t->hpose + t->q_T, in->Twc_h, 56 * (size_t)n_active);
    memcpy(t->hpose + t->q_seed, in->seed_h, 8 * (size_t)n_active);
    uint8_t *fl = t->hpose + t->q_fl;
    for (int b = 0; b < n_active; b++) {
        const int req = in->p3p_req_h[b] != 0;
        fl[b] = (uint8_t)(req | ((req || pp->dop3p) ? 2 : 0));
        const size_t n = (size_t)n_h[b], o = (size_t)b * nm;
        int *sc = (int *)(t->hpose + t->q_sc) + o;
        if (in->scale_h) memcpy(sc, in->scale_h + o, 4 * n); else memset(sc, 0, 4 * n);
    }
    return OV2_OK;
}

// what an epipolar + pose step refuses beyond the pose step's checks; *L: the filter's layout at capacity
static int check_epi(const ov2_btracker *t, const ov2_frame_epi_pose_params *pp, const ov2_frame_epi_pose_input *in, EpifLayout *L)
{
    OV2_REQUIRE(pp && in, OV2_EINVAL, "ov2_btracker_track_frame_epi_pose: NULL params / input");
    OV2_REQUIRE(in->lmid_h && in->nbkfs_h && in->epi_seed_h, OV2_EINVAL, "ov2_btracker_track_frame_epi_pose: NULL lmid_h / nbkfs_h / epi_seed_h");
    const int rc = epif_check_params(&pp->epi);  if (rc) return rc;
    OV2_REQUIRE(t->cfg.n_max <= OV2_FKF_MAX_POINTS, OV2_EINVAL, "capacity: cfg.n_max exceeds OV2_FKF_MAX_POINTS (2048) keypoints of one frame");
    return epif_layout_capacity(t->batch, t->cfg.n_max, pp->epi.n_rows, L);
}

// The epipolar side's buffers (allocated by the first call) and the filter's block, grown to hold layout L.  The keyframe arrays lie
// in the block's input section, whose offsets do not depend on the rows: a grown block gets them again from the host copy.
static int ensure_epi(ov2_btracker *t, const EpifLayout *L)
{
    const size_t nm = (size_t)t->cfg.n_max, B = (size_t)t->batch, slots = nm * B;
    OV2_HIP_CHECK(hipSetDevice(t->ctx->device));
    if (!t->hepi) {
        EpifLayout L0;
        const int rc = epif_layout_capacity(t->batch, t->cfg.n_max, 0, &L0);  if (rc) return rc;
        t->e_lm = 0; t->e_nk = up256(4 * slots); t->e_sd = up256(t->e_nk + 4 * B); t->e_in = up256(t->e_sd + 8 * B);
        t->e_out = t->e_in; t->e_nc = up256(t->e_out + sizeof(EpifOut) * B); t->e_rm = up256(t->e_nc + 4 * B);
        t->e_er = up256(t->e_rm + slots); t->e_pc = up256(t->e_er + 4 * slots); t->epi_bytes = up256(t->e_pc + 4 * slots);
        t->x_slot = up256(sizeof(FeKfHdr) * B); t->x_rank = t->x_slot + 4 * slots;
        const size_t fx_bytes = t->x_rank + 4 * slots;
        uint8_t *h = nullptr, *d = nullptr, *fx = nullptr;
        hipError_t e = hipHostMalloc((void **)&h, t->epi_bytes, hipHostMallocMapped);
        if (e == hipSuccess && !t->zero_copy) e = hipMalloc((void **)&d, t->epi_bytes);
        void *alias = d;
        if (e == hipSuccess && t->zero_copy) e = hipHostGetDevicePointer(&alias, h, 0);
        if (e == hipSuccess) e = hipMalloc((void **)&fx, fx_bytes);
        if (e == hipSuccess) e = hipMemsetAsync(fx, 0, fx_bytes, t->ctx->stream);       // no item has a keyframe yet
        if (e == hipSuccess) e = hipStreamSynchronize(t->ctx->stream);
        if (e != hipSuccess || !alias) {
            if (h) (void)hipHostFree(h);
            if (d) (void)hipFree(d);
            if (fx) (void)hipFree(fx);
            (void)hipGetLastError();
            ov2_set_error("ov2_btracker_track_frame_epi_pose: %s", hipGetErrorString(e));
            return OV2_ENOMEM;
        }
        memset(h, 0, t->epi_bytes);
        t->hepi = h; t->depi_io = d; t->kepi = (uint8_t *)alias; t->dfx = fx;
        t->eL0 = L0;
        t->kf_host.assign(L0.o_up - L0.o_kl, 0);
        t->kf_hdr.assign(B, FeKfHdr());
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
            ov2_set_error("ov2_btracker_track_frame_epi_pose: %s", hipGetErrorString(e));
            return OV2_ENOMEM;
        }
        if (t->depi) (void)hipFree(t->depi);
        t->depi = nd; t->depi_bytes = need; t->le_on = false;           // the lists of the last step go with the block
    }
    return OV2_OK;
}

// the filter's inputs of a step into hepi
static void stage_epi(ov2_btracker *t, int n_active, const ov2_frame_epi_pose_input *in, const int *n_h)
{
    const size_t nm = (size_t)t->cfg.n_max;
    for (int b = 0; b < n_active; b++)
        if (n_h[b] > 0) memcpy(t->hepi + t->e_lm + 4 * nm * (size_t)b, in->lmid_h + nm * (size_t)b, 4 * (size_t)n_h[b]);
    memcpy(t->hepi + t->e_nk, in->nbkfs_h, 4 * (size_t)n_active);
    memcpy(t->hepi + t->e_sd, in->epi_seed_h, 8 * (size_t)n_active);
}

static void stage_points(ov2_btracker *t, int n_active, const float *kps, const float *pri, const uint8_t *has_prior, const int *n_h, int use_prior)
{
    const size_t nm = (size_t)t->cfg.n_max;
    int *nd = (int *)(t->hblk + t->o_n);
    for (int b = 0; b < t->batch; b++) nd[b] = b < n_active ? n_h[b] : 0;
    for (int b = 0; b < n_active; b++) {
        const size_t n = (size_t)n_h[b], o = (size_t)b * nm;
        if (!n) continue;
        memcpy(t->hblk + t->o_kps + 8 * o, kps + 2 * o, 8 * n);
        if (!pri) continue;                                              // the map form: k_prior_frame writes both
        memcpy(t->hblk + t->o_pri + 8 * o, pri + 2 * o, 8 * n);
        uint8_t *f = t->hblk + t->o_flg + o;
        if (use_prior && has_prior) for (size_t i = 0; i < n; i++) f[i] = has_prior[o + i] ? 1 : 0;
        else memset(f, 0, n);
    }
}

// the cross-keypoint rule of visual_front_end.cpp:225-230 for item b (same as track.hip: apply_p3p_rule), on the item's views
static int apply_p3p_rule(ov2_btracker *t, int b, const float *kps, const uint8_t *has_prior, int use_prior, int n, float *out_xy,
                          uint8_t *status, int *p3p_req)
{
    size_t nbkps = 0, nbgood = 0;
    if (use_prior && has_prior)
        for (int i = 0; i < n; i++) if (has_prior[i]) { nbkps++; if ((status[i] & 3) == 1) nbgood++; }
    int p3p = 0;
    if (nbkps > 0 && (double)nbgood < 0.33 * (double)nbkps) {
        p3p = 1;                                                        // vpriors = vkps for the second call (:229)
        std::vector<int> idx;
        for (int i = 0; i < n; i++) if (status[i] & 2) idx.push_back(i);
        if (!idx.empty()) {
            const int m = (int)idx.size();
            std::vector<float> k2(2 * (size_t)m), p2(2 * (size_t)m);
            std::vector<uint8_t> s2((size_t)m);
            for (int j = 0; j < m; j++) { k2[2 * j] = p2[2 * j] = kps[2 * idx[j]]; k2[2 * j + 1] = p2[2 * j + 1] = kps[2 * idx[j] + 1]; }
            const ov2_tracker_config &c = t->cfg;
            const int rc = ov2_fb_klt(t->ctx, t->view[t->prev()][b], t->view[t->cur][b], c.win, c.nklt_pyr_lvl, c.max_iter, c.eps, c.err_th,
                                      c.fb_dist, k2.data(), p2.data(), m, s2.data(), nullptr);
            if (rc != OV2_OK) return rc;
            for (int j = 0; j < m; j++) {
                out_xy[2 * idx[j]] = p2[2 * j]; out_xy[2 * idx[j] + 1] = p2[2 * j + 1];
                status[idx[j]] = (uint8_t)(2 | (s2[j] ? 1 : 0));
            }
            if (t->has_calib) {                                        // their undistorted pixels / bearings follow the new positions
                std::vector<float> u2(2 * (size_t)m);
                std::vector<double> b2(3 * (size_t)m);
                const KpCalib &kc = t->calib;
                const double Kk[4] = {kc.fx, kc.fy, kc.cx, kc.cy};
                const int rck = ov2_compute_keypoints(t->ctx, kc.model, Kk, kc.nD ? kc.k : nullptr, kc.nD, kc.iK, p2.data(), m, u2.data(), b2.data());
                if (rck != OV2_OK) return rck;
                float *un = (float *)(t->hblk + t->o_unpx) + 2 * (size_t)b * t->cfg.n_max;
                double *bv = (double *)(t->hblk + t->o_bv) + 3 * (size_t)b * t->cfg.n_max;
                for (int j = 0; j < m; j++) {
                    memcpy(un + 2 * (size_t)idx[j], &u2[2 * (size_t)j], 8);
                    memcpy(bv + 3 * (size_t)idx[j], &b2[3 * (size_t)j], 24);
                }
            }
        }
    }
    if (p3p_req) *p3p_req = p3p;
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
    int *nh = (int *)t->h_det;
    for (int b = 0; b < n_active; b++) {
        const int n = ncur_h ? ncur_h[b] : 0;
        OV2_REQUIRE(n >= 0 && (size_t)n <= nm && (n == 0 || cur_xy_h), OV2_EINVAL, "bad current keypoints");
        nh[b] = n;
        if (n) memcpy(t->h_det + o_cur + 8 * nm * b, cur_xy_h + 2 * nm * b, 8 * (size_t)n);
    }
    if (out_cap > t->out_cap) {                                          // grow-only result mirrors
        OV2_HIP_CHECK(hipStreamSynchronize(ctx->stream));
        if (t->d_out) (void)hipFree(t->d_out);
        if (t->h_out) (void)hipHostFree(t->h_out);
        t->d_out = nullptr; t->h_out = nullptr; t->out_cap = 0;
        OV2_HIP_CHECK(hipMalloc((void **)&t->d_out, 8 * (size_t)out_cap * t->batch));
        OV2_HIP_CHECK(hipHostMalloc((void **)&t->h_out, 8 * (size_t)out_cap * t->batch, hipHostMallocDefault));
        t->out_cap = out_cap;
    }
    OV2_HIP_CHECK(hipMemcpyAsync(t->d_det, t->h_det, o_cur + 8 * nm * (size_t)n_active, hipMemcpyHostToDevice, ctx->stream));
    const ov2_pyr q = prefix_of(t->pyr[t->cur], n_active);
    const float *cur_d = (const float *)(t->d_det + o_cur);
    const int *ncur_d = (const int *)t->d_det;
    if (mode == 2 && roi_h) {
        OV2_REQUIRE(roi_stride >= t->cfg.w, OV2_EINVAL, "roi stride < width");
        if (!t->d_roi) OV2_HIP_CHECK(hipMalloc((void **)&t->d_roi, (size_t)t->cfg.w * t->cfg.h));
        OV2_HIP_CHECK(hipMemcpy2DAsync(t->d_roi, (size_t)t->cfg.w, roi_h, (size_t)roi_stride, (size_t)t->cfg.w, (size_t)t->cfg.h,
                                       hipMemcpyHostToDevice, ctx->stream));
    }
    int rc;
    if (mode == 2) rc = ov2_detect_gftt_batch_d(ctx, &q, roi_h ? t->d_roi : nullptr, t->cfg.w, gp, cur_d, (int)nm, ncur_d, nbmax_h, do_subpix,
                                                t->d_out, t->out_cap, out_n_h);
    else if (mode == 0) rc = ov2_detect_grid_fast_batch_d(ctx, &q, cell, cur_d, (int)nm, ncur_d, fast_th_inout, mask_mode, do_subpix, t->d_out, t->out_cap, out_n_h);
    else rc = ov2_detect_singlescale_batch_d(ctx, &q, cell, cur_d, (int)nm, ncur_d, roi, quality_inout, do_subpix, t->d_out, t->out_cap, out_n_h);
    if (rc != OV2_OK) return rc;
    OV2_HIP_CHECK(hipMemcpyAsync(t->h_out, t->d_out, 8 * (size_t)t->out_cap * n_active, hipMemcpyDeviceToHost, ctx->stream));
    OV2_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    for (int b = 0; b < n_active; b++)
        if (out_n_h[b] > 0) memcpy(out_xy_h + 2 * (size_t)out_cap * b, t->h_out + 8 * (size_t)t->out_cap * b, 8 * (size_t)out_n_h[b]);
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
    t->img_pitch = up16((size_t)cfg->w);
    t->img_bytes = up256(t->img_pitch * (size_t)cfg->h);
    const size_t nm = (size_t)cfg->n_max * (size_t)batch;
    t->o_n = 0; t->o_kps = up256(4 * (size_t)batch); t->o_pri = t->o_kps + 8 * nm; t->o_flg = t->o_pri + 8 * nm; t->in_bytes = up256(t->o_flg + nm);
    t->o_out = t->in_bytes; t->o_st = t->o_out + 8 * nm; t->o_unpx = up256(t->o_st + nm); t->o_bv = up256(t->o_unpx + 8 * nm); t->blk_bytes = t->o_bv + 24 * nm;
    t->det_in_bytes = up256(4 * (size_t)batch) + 8 * nm;
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
    if (e == hipSuccess) e = hipHostMalloc((void **)&t->hblk, t->blk_bytes, hipHostMallocMapped);
    if (e == hipSuccess) e = hipMalloc((void **)&t->dblk, t->blk_bytes);
    if (e == hipSuccess) e = hipMemsetAsync(t->dblk, 0, t->blk_bytes, ctx->stream);
    if (e == hipSuccess) e = hipHostMalloc((void **)&t->h_det, t->det_in_bytes, hipHostMallocDefault);
    if (e == hipSuccess) e = hipMalloc((void **)&t->d_det, t->det_in_bytes);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) { ov2_set_error("ov2_btracker_create: %s", hipGetErrorString(e)); btracker_free(t); return OV2_ENOMEM; }
    memset(t->hblk, 0, t->blk_bytes);
    memset(t->h_det, 0, t->det_in_bytes);
    t->side.device = ctx->device; t->side.stream = t->ps; t->side.owns_stream = false;
    t->kblk = t->dblk;
    {   // the kernels read / write the pinned block through its device alias (no staging copies); the device block is the fallback
        void *alias = nullptr;
        if (hipHostGetDevicePointer(&alias, t->hblk, 0) == hipSuccess && alias) { t->kblk = (uint8_t *)alias; t->zero_copy = true; }
        else (void)hipGetLastError();
    }
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
    OV2_REQUIRE(t->prepq.empty() && !t->pend.on, OV2_EINVAL, "ov2_btracker_set_rectification between steps only: prepared frames wait or a step is open");
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

// the forms of the step's first half.  map: the priors come from the device (wpt_h / is3d_h / Tcw_h), prior_xy_h / has_prior_h are unused;
// pose (a map form): the pose of ov2_btracker_track_frame_pose follows in the same enqueue
static int track_frame_begin(ov2_btracker *t, int n_active, const uint8_t *const *img_h, int stride, const float *kps_xy_h,
                             const float *prior_xy_h, const uint8_t *has_prior_h, const int *n_h, int klt_use_prior, bool map,
                             const double *wpt_h, const uint8_t *is3d_h, const double *Tcw_h, bool pose = false,
                             const ov2_frame_pose_params *pp = nullptr, const ov2_frame_pose_input *pin = nullptr, bool epi = false,
                             const ov2_frame_epi_pose_params *epp = nullptr, const ov2_frame_epi_pose_input *ein = nullptr)
{
    OV2_REQUIRE(t && img_h, OV2_EINVAL, "NULL argument");
    OV2_REQUIRE(!map || t->has_calib, OV2_EINVAL, "ov2_btracker_track_frame_map: no calibration set on this tracker");
    OV2_REQUIRE(!t->pend.on, OV2_EINVAL, "ov2_btracker_track_frame_begin: the previous step has not been finished (ov2_btracker_track_frame_end)");
    OV2_REQUIRE(n_active >= 1 && n_active <= t->batch, OV2_EINVAL, "n_active out of range");
    OV2_REQUIRE(stride >= t->cfg.w, OV2_EINVAL, "stride < width");
    const size_t nm = (size_t)t->cfg.n_max;
    int n_total = 0;
    for (int b = 0; b < n_active; b++) {
        OV2_REQUIRE(img_h[b] != nullptr, OV2_EINVAL, "NULL frame of an active item");
        const int n = n_h ? n_h[b] : 0;
        OV2_REQUIRE(n >= 0 && (size_t)n <= nm, OV2_EINVAL, "an item carries more keypoints than cfg.n_max slots");
        n_total += n;
    }
    if (map) OV2_REQUIRE(n_total == 0 || (kps_xy_h && wpt_h && is3d_h && Tcw_h && n_h), OV2_EINVAL, "NULL point buffer");
    else OV2_REQUIRE(n_total == 0 || (kps_xy_h && prior_xy_h && n_h), OV2_EINVAL, "NULL point buffer");
    PoseLayout poseL;
    EpifLayout epiL;
    if (epi) {                                                           // (pp / pin: the pose halves of epp / ein, or NULL with them)
        OV2_REQUIRE(epp && ein, OV2_EINVAL, "ov2_btracker_track_frame_epi_pose: NULL params / input");
        pp = &epp->pose; pin = &ein->pose;
    }
    if (pose) { const int rcp = check_pose(t, n_active, wpt_h, is3d_h, n_h, pp, pin, &poseL);  if (rcp != OV2_OK) return rcp; }
    if (epi) { const int rce = check_epi(t, epp, ein, &epiL);  if (rce != OV2_OK) return rce; }
    for (int b = 0; b < t->batch; b++) t->last_n[(size_t)b] = t->last_pn[(size_t)b] = 0;
    ov2_ctx *ctx = t->ctx;
    OV2_HIP_CHECK(hipSetDevice(ctx->device));
    int which = 0;
    bool prepared = false;
    t->raw_which = -1;                                                   // staging may rewrite any set
    int rc = stage_and_upload(t, n_active, img_h, stride, &which, &prepared);
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
    P.n_active = n_active; P.use_prior = klt_use_prior; P.kps = kps_xy_h; P.has_prior = has_prior_h;
    P.n.assign((size_t)n_active, 0);
    if (n_h) for (int b = 0; b < n_active; b++) P.n[(size_t)b] = n_h[b];
    P.pose = pose;
    if (pose) {
        P.pp = *pp; P.L = poseL;
        P.Twc.assign(pin->Twc_h, pin->Twc_h + 7 * (size_t)n_active);
        P.req.assign(pin->p3p_req_h, pin->p3p_req_h + n_active);
        P.seed.assign(pin->seed_h, pin->seed_h + n_active);
    }
    P.epi = epi;
    if (epi) { P.ep = epp->epi; P.eL = epiL; }
    if (t->frames == 0 || n_total == 0) {
        // first frame (trackMono returns right after preprocessImage) or nothing to track anywhere
        rc = preprocess();
        if (rc != OV2_OK) { t->cur = old_cur; return rc; }
        commit();
        P.tracked = false; P.on = true;
        return OV2_OK;
    }
    if (map) {
        rc = stage_map(t, n_active, wpt_h, is3d_h, Tcw_h, n_h);
        if (rc != OV2_OK) { t->cur = old_cur; return rc; }
        P.has_prior = t->hblk + t->o_flg;                                // the flags the device sets: same slots as the caller's array
    }
    if (pose) {
        rc = stage_pose(t, n_active, pp, pin, n_h, poseL);
        if (rc != OV2_OK) { t->cur = old_cur; return rc; }
    }
    if (epi) {
        rc = ensure_epi(t, &epiL);
        if (rc != OV2_OK) { t->cur = old_cur; return rc; }
        stage_epi(t, n_active, ein, n_h);
    }
    stage_points(t, n_active, kps_xy_h, map ? nullptr : prior_xy_h, has_prior_h, n_h, klt_use_prior);
    rc = preprocess();
    if (rc == OV2_OK) rc = enqueue_klt(t, t->pyr[t->prev()], t->pyr[t->cur], n_active, map ? (klt_use_prior ? 1 : 0) : -1, pose ? &P : nullptr);
    if (rc != OV2_OK) { t->cur = old_cur; return rc; }
    commit();
    P.tracked = true; P.on = true;
    return OV2_OK;
}

extern "C" {

int ov2_btracker_track_frame_begin(ov2_btracker *t, int n_active, const uint8_t *const *img_h, int stride, const float *kps_xy_h,
                                   const float *prior_xy_h, const uint8_t *has_prior_h, const int *n_h, int klt_use_prior)
{
    return track_frame_begin(t, n_active, img_h, stride, kps_xy_h, prior_xy_h, has_prior_h, n_h, klt_use_prior, false, nullptr, nullptr, nullptr);
}

int ov2_btracker_track_frame_map_begin(ov2_btracker *t, int n_active, const uint8_t *const *img_h, int stride, const float *kps_xy_h,
                                       const double *wpt_h, const uint8_t *is3d_h, const double *Tcw_h, const int *n_h, int klt_use_prior)
{
    return track_frame_begin(t, n_active, img_h, stride, kps_xy_h, nullptr, nullptr, n_h, klt_use_prior, true, wpt_h, is3d_h, Tcw_h);
}

} // extern "C"

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

// The items where the 33 % rule fired (`redo`), after their retry: the pose set from the final status, the step's unpx / bv as the
// retry left them, a table drawn from the new m, and ov2_compute_pose_batch over just those items with do_p3p = p3p_req = 1
// excl (or NULL): one byte per slot, laid out like status_h -- a slot the filter removed is not in the pose set
static int pose_redo(ov2_btracker *t, const std::vector<int> &redo, const uint8_t *status_h, ov2_pose_result *results,
                     const uint8_t *excl = nullptr)
{
    const ov2_btracker::Pending &P = t->pend;
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
        const float *un = (const float *)(t->hblk + t->o_unpx) + 2 * o;
        const double *bvs = (const double *)(t->hblk + t->o_bv) + 3 * o, *w = (const double *)(t->hmap + t->m_w) + 3 * o;
        const uint8_t *d3 = t->hmap + t->m_3d + o;
        const int *sc = (const int *)(t->hpose + t->q_sc) + o;
        std::vector<int> &slot = t->lp_slot[(size_t)b];
        slot.clear();
        for (int i = 0; i < n; i++)
            if ((status_h[o + i] & 3) == 1 && d3[i] && !(excl && excl[o + i])) {
                slot.push_back(i);
                unpx[k].push_back((double)un[2 * i]); unpx[k].push_back((double)un[2 * i + 1]);
                for (int c = 0; c < 3; c++) { wpt[k].push_back(w[3 * i + c]); bv[k].push_back(bvs[3 * i + c]); }
                scale[k].push_back(sc[i]);
            }
        const int m = (int)slot.size();
        std::vector<int> &tab = t->lp_samples[(size_t)b];
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
        t->lp_m[(size_t)b] = m; t->lp_rows[(size_t)b] = q.n_rows; t->lp_host[(size_t)b] = 1;
    }
    const int rc = ov2_compute_pose_batch(t->ctx, &P.pp.pose, (int)R, pb.data(), rs.data());
    if (rc != OV2_OK) return rc;
    for (size_t k = 0; k < R; k++) {
        const int b = redo[k];
        ov2_pose_result &r = results[b];
        uint8_t *removed = r.removed;
        r = rs[k];
        r.removed = removed;
        if (P.n[(size_t)b] > 0) memset(removed, 0, (size_t)P.n[(size_t)b]);
        const std::vector<int> &slot = t->lp_slot[(size_t)b];
        for (size_t j = 0; j < slot.size(); j++) removed[slot[j]] = rm[k][j];
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
    const EpifLayout &L0 = t->eL0;
    const uint8_t *kh = t->kf_host.data();
    const int *lmid_h = (const int *)(t->hepi + t->e_lm), *nbkfs_h = (const int *)(t->hepi + t->e_nk);    // as the step staged them
    const unsigned long long *seed_h = (const unsigned long long *)(t->hepi + t->e_sd);
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
        const float *un = (const float *)(t->hblk + t->o_unpx) + 2 * o;
        const double *bvs = (const double *)(t->hblk + t->o_bv) + 3 * o;
        const uint8_t *f3 = t->hmap + t->m_3d + o;
        std::vector<int> &slot = t->le_slot[(size_t)b];
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
        std::vector<int> &tab = t->le_samples[(size_t)b];
        tab.assign(8 * (size_t)(n_rows > 0 ? n_rows : 1), -1);
        const FeKfHdr &h = t->kf_hdr[(size_t)b];
        ov2_epifilter_item &q = items[k];
        memset(&q, 0, sizeof q);
        q.fkf.n_cur = nc; q.fkf.cur_lmid = lmid[k].data(); q.fkf.cur_px = px[k].data(); q.fkf.cur_unpx = unpx[k].data();
        q.fkf.cur_bv = bv[k].data(); q.fkf.cur_is3d = d3[k].data(); q.fkf.cur_Twc = P.Twc.data() + 7 * (size_t)b;
        q.fkf.n_kf = h.n_kf; q.fkf.kf_lmid = (const int *)kh + o; q.fkf.kf_unpx = (const float *)(kh + (L0.o_ku - L0.o_kl)) + 2 * o;
        q.fkf.kf_Tcw = h.kf_Tcw; q.fkf.noccupcells = -1; q.fkf.nb3dkps = -1;
        q.kf_bv = (const double *)(kh + (L0.o_kb - L0.o_kl)) + 3 * o; q.kf_Twc = h.kf_Twc; q.nbkfs = nbkfs_h[b]; q.seed = seed_h[b];
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
        const std::vector<int> &slot = t->le_slot[(size_t)b];
        ov2_epifilter_result &r = results[b], keep = results[b];
        r = rs[k];
        r.removed = keep.removed; r.pair_cur = keep.pair_cur; r.err = keep.err; r.trace_samples = nullptr;
        if (n > 0) memset(r.removed, 0, (size_t)n);
        if (r.err && n > 0) memset(r.err, 0, 4 * (size_t)n);
        for (size_t j = 0; j < slot.size(); j++) {
            r.removed[slot[j]] = rm[k][j];
            if (r.err) r.err[slot[j]] = err[k][j];
            if (rm[k][j]) excl[o + (size_t)slot[j]] = 1;
        }
        if (r.pair_cur)
            for (int j = 0; j < r.m && j < (int)slot.size(); j++)
                r.pair_cur[j] = (unsigned)pair[k][(size_t)j] < slot.size() ? slot[(size_t)pair[k][(size_t)j]] : -1;
        t->le_ncur[(size_t)b] = (int)slot.size(); t->le_m[(size_t)b] = r.m;
        t->le_rows[(size_t)b] = epi_rows_used(r.action, r.m, n_rows); t->le_host[(size_t)b] = 1;
    }
    return OV2_OK;
}

// both forms of the step's second half.  results != NULL: the step was begun with ov2_btracker_track_frame_pose_begin and its
// poses are wanted; NULL: the tracking half only (a pose the step computed is dropped)
// eres != NULL (with results): the step was begun with ov2_btracker_track_frame_epi_pose_begin and the filter's records are wanted too
static int track_frame_end(ov2_btracker *t, float *out_xy_h, uint8_t *status_h, int *p3p_req, ov2_pose_result *results,
                           ov2_epifilter_result *eres = nullptr)
{
    OV2_REQUIRE(t, OV2_EINVAL, "NULL tracker");
    ov2_btracker::Pending &P = t->pend;
    OV2_REQUIRE(P.on, OV2_EINVAL, "ov2_btracker_track_frame_end without ov2_btracker_track_frame_begin");
    OV2_REQUIRE(!results || P.pose, OV2_EINVAL, "ov2_btracker_track_frame_pose_end: the step was not begun with ov2_btracker_track_frame_pose_begin");
    if (results)
        for (int b = 0; b < P.n_active; b++)
            OV2_REQUIRE(P.n[(size_t)b] == 0 || results[b].removed, OV2_EINVAL, "NULL result buffer (removed)");
    OV2_REQUIRE(!eres || P.epi, OV2_EINVAL, "ov2_btracker_track_frame_epi_pose_end: the step was not begun with ov2_btracker_track_frame_epi_pose_begin");
    OV2_REQUIRE(!results || !P.epi || eres, OV2_EINVAL, "ov2_btracker_track_frame_pose_end: the step was begun with ov2_btracker_track_frame_epi_pose_begin");
    if (eres)
        for (int b = 0; b < P.n_active; b++) {
            OV2_REQUIRE(P.n[(size_t)b] == 0 || eres[b].removed, OV2_EINVAL, "NULL result buffer (removed) of the filter");
            OV2_REQUIRE(!eres[b].trace_samples, OV2_EINVAL, "trace_samples must be NULL in a step: ov2_btracker_last_epi_inputs fetches the table");
        }
    P.on = false;
    if (results) {
        const size_t B = (size_t)t->batch;
        t->lp_on = true; t->lp_chain = P.tracked; t->lp_L = P.L;
        t->lp_m.assign(B, 0); t->lp_rows.assign(B, 0); t->lp_host.assign(B, 0);
        t->lp_slot.resize(B); t->lp_samples.resize(B);
        if (!P.tracked)                                                  // first frame / nothing tracked: no chain ran
            for (int b = 0; b < P.n_active; b++) {
                ov2_pose_result &r = results[b];
                uint8_t *removed = r.removed;
                memset(&r, 0, sizeof(r));
                r.removed = removed;
                if (P.n[(size_t)b] > 0) memset(removed, 0, (size_t)P.n[(size_t)b]);
                memcpy(r.Twc, P.Twc.data() + 7 * (size_t)b, 56);
                r.action = OV2_POSE_TOO_FEW; r.p3p_req_out = P.req[(size_t)b] != 0;
            }
    }
    if (eres) {
        const size_t B = (size_t)t->batch;
        t->le_on = true; t->le_chain = P.tracked; t->le_L = P.eL;
        t->le_ncur.assign(B, 0); t->le_m.assign(B, 0); t->le_rows.assign(B, 0); t->le_host.assign(B, 0);
        t->le_slot.resize(B); t->le_samples.resize(B);
        if (!P.tracked)                                                  // first frame / nothing tracked: no chain ran
            for (int b = 0; b < P.n_active; b++) {
                ov2_epifilter_result &r = eres[b], keep = eres[b];
                memset(&r, 0, sizeof(r));
                r.removed = keep.removed; r.pair_cur = keep.pair_cur; r.err = keep.err;
                r.action = OV2_EPIF_TOO_FEW_KPS;
                if (P.n[(size_t)b] > 0) memset(r.removed, 0, (size_t)P.n[(size_t)b]);
                if (P.n[(size_t)b] > 0 && r.err) memset(r.err, 0, 4 * (size_t)P.n[(size_t)b]);
            }
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
    std::vector<int> rule((size_t)P.n_active, 0);
    for (int b = 0; b < P.n_active; b++) {
        const size_t n = (size_t)P.n[(size_t)b], o = nm * (size_t)b;
        if (!n) continue;
        memcpy(out_xy_h + 2 * o, t->hblk + t->o_out + 8 * o, 8 * n);
        memcpy(status_h + o, t->hblk + t->o_st + o, n);
        const int rc = apply_p3p_rule(t, b, P.kps + 2 * o, P.has_prior ? P.has_prior + o : nullptr, P.use_prior, (int)n, out_xy_h + 2 * o,
                                      status_h + o, &rule[(size_t)b]);
        if (rc != OV2_OK) return rc;
        if (p3p_req) p3p_req[b] = rule[(size_t)b];
        if (t->has_calib) t->last_n[(size_t)b] = (int)n;
        t->last_pn[(size_t)b] = (int)n;
    }
    if (!results) return OV2_OK;
    std::vector<int> redo;
    for (int b = 0; b < P.n_active; b++) {
        const size_t n = (size_t)P.n[(size_t)b], o = nm * (size_t)b;
        int ms[2];
        memcpy(ms, t->hpose + t->q_ms + 8 * (size_t)b, 8);
        t->lp_m[(size_t)b] = ms[0]; t->lp_rows[(size_t)b] = ms[1];
        if (n && rule[(size_t)b]) { redo.push_back(b); continue; }
        if (eres) {
            ov2_epifilter_result &r = eres[b];
            EpifOut eo;
            memcpy(&eo, t->hepi + t->e_out + sizeof(EpifOut) * (size_t)b, sizeof(EpifOut));
            epi_store(r, eo);
            memcpy(&t->le_ncur[(size_t)b], t->hepi + t->e_nc + 4 * (size_t)b, 4);
            t->le_m[(size_t)b] = eo.m; t->le_rows[(size_t)b] = epi_rows_used(eo.action, eo.m, P.ep.n_rows);
            if (n) {
                memcpy(r.removed, t->hepi + t->e_rm + o, n);
                if (r.pair_cur && eo.m > 0) memcpy(r.pair_cur, t->hepi + t->e_pc + 4 * o, 4 * (size_t)(eo.m < (int)n ? eo.m : (int)n));
                if (r.err) memcpy(r.err, t->hepi + t->e_er + 4 * o, 4 * n);
            }
        }
        PoseOut po;
        memcpy(&po, t->hpose + t->q_out + sizeof(PoseOut) * (size_t)b, sizeof(PoseOut));
        pose_store(results[b], po);
        if (n) memcpy(results[b].removed, t->hpose + t->q_rm + o, n);
    }
    if (!redo.empty() && eres) {
        std::vector<uint8_t> excl;
        const int rc = epi_redo(t, redo, out_xy_h, status_h, eres, excl);
        if (rc != OV2_OK) return rc;
        return pose_redo(t, redo, status_h, results, excl.data());
    }
    if (!redo.empty()) return pose_redo(t, redo, status_h, results);
    return OV2_OK;
}

extern "C" {

int ov2_btracker_track_frame_end(ov2_btracker *t, float *out_xy_h, uint8_t *status_h, int *p3p_req)
{
    return track_frame_end(t, out_xy_h, status_h, p3p_req, nullptr);
}

int ov2_btracker_track_frame_pose_begin(ov2_btracker *t, int n_active, const uint8_t *const *img_h, int stride, const float *kps_xy_h,
                                        const double *wpt_h, const uint8_t *is3d_h, const double *Tcw_h, const int *n_h,
                                        int klt_use_prior, const ov2_frame_pose_params *params, const ov2_frame_pose_input *input)
{
    return track_frame_begin(t, n_active, img_h, stride, kps_xy_h, nullptr, nullptr, n_h, klt_use_prior, true, wpt_h, is3d_h, Tcw_h,
                             true, params, input);
}

int ov2_btracker_track_frame_pose_end(ov2_btracker *t, float *out_xy_h, uint8_t *status_h, int *p3p_req, ov2_pose_result *results)
{
    OV2_REQUIRE(results, OV2_EINVAL, "NULL result array");
    return track_frame_end(t, out_xy_h, status_h, p3p_req, results);
}

int ov2_btracker_track_frame_pose(ov2_btracker *t, int n_active, const uint8_t *const *img_h, int stride, const float *kps_xy_h,
                                  const double *wpt_h, const uint8_t *is3d_h, const double *Tcw_h, const int *n_h, int klt_use_prior,
                                  const ov2_frame_pose_params *params, const ov2_frame_pose_input *input,
                                  float *out_xy_h, uint8_t *status_h, int *p3p_req, ov2_pose_result *results)
{
    OV2_REQUIRE(results, OV2_EINVAL, "NULL result array");
    if (t && n_active >= 1 && n_active <= t->batch && n_h) {              // as ov2_btracker_track_frame: the result buffers before anything is enqueued
        int n_total = 0;
        for (int b = 0; b < n_active; b++) {
            n_total += n_h[b] > 0 ? n_h[b] : 0;
            OV2_REQUIRE(n_h[b] <= 0 || results[b].removed, OV2_EINVAL, "NULL result buffer (removed)");
        }
        OV2_REQUIRE(n_total == 0 || (out_xy_h && status_h), OV2_EINVAL, "NULL point buffer");
    }
    const int rc = ov2_btracker_track_frame_pose_begin(t, n_active, img_h, stride, kps_xy_h, wpt_h, is3d_h, Tcw_h, n_h, klt_use_prior, params, input);
    if (rc != OV2_OK) return rc;
    return track_frame_end(t, out_xy_h, status_h, p3p_req, results);
}

int ov2_btracker_last_pose_inputs(const ov2_btracker *t, int item, int *m, int *slot_idx, int *samples, int *n_rows_used)
{
    OV2_REQUIRE(t, OV2_EINVAL, "NULL tracker");
    OV2_REQUIRE(item >= 0 && item < t->batch, OV2_EINVAL, "batch item out of range");
    OV2_REQUIRE(t->lp_on, OV2_EINVAL, "ov2_btracker_last_pose_inputs: no pose step has been finished on this tracker");
    const size_t b = (size_t)item;
    const int mm = t->lp_m[b], rows = t->lp_rows[b];
    if (m) *m = mm;
    if (n_rows_used) *n_rows_used = rows;
    if (t->lp_host[b]) {
        if (slot_idx && mm > 0) memcpy(slot_idx, t->lp_slot[b].data(), 4 * (size_t)mm);
        if (samples && rows > 0) memcpy(samples, t->lp_samples[b].data(), 16 * (size_t)rows);
        return OV2_OK;
    }
    if (!t->lp_chain || (mm <= 0 && rows <= 0)) return OV2_OK;
    OV2_HIP_CHECK(hipSetDevice(t->ctx->device));
    const PoseLayout &L = t->lp_L;
    if (slot_idx && mm > 0)
        OV2_HIP_CHECK(hipMemcpy(slot_idx, t->dwork + ov2_frame_pose_slot_offset(L) + 4 * b * (size_t)L.n_max, 4 * (size_t)mm, hipMemcpyDeviceToHost));
    if (samples && rows > 0)
        OV2_HIP_CHECK(hipMemcpy(samples, t->dwork + L.o_p3 + L.pl.o_sm + 16 * b * (size_t)L.n_rows, 16 * (size_t)rows, hipMemcpyDeviceToHost));
    return OV2_OK;
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
    OV2_REQUIRE(!t->pend.on, OV2_EINVAL, "ov2_btracker_set_keyframe between steps only: a step is open");
    const int rc = ensure_epi(t, nullptr);
    if (rc != OV2_OK) return rc;
    const EpifLayout &L0 = t->eL0;
    const size_t o = (size_t)item * (size_t)t->cfg.n_max, n = (size_t)n_kf;
    uint8_t *kh = t->kf_host.data();
    hipStream_t s = t->ctx->stream;
    if (n) {
        memcpy(kh + 4 * o, kf_lmid, 4 * n);
        memcpy(kh + (L0.o_ku - L0.o_kl) + 8 * o, kf_unpx, 8 * n);
        memcpy(kh + (L0.o_kb - L0.o_kl) + 24 * o, kf_bv, 24 * n);
        OV2_HIP_CHECK(hipMemcpyAsync(t->depi + L0.o_kl + 4 * o, kh + 4 * o, 4 * n, hipMemcpyHostToDevice, s));
        OV2_HIP_CHECK(hipMemcpyAsync(t->depi + L0.o_ku + 8 * o, kh + (L0.o_ku - L0.o_kl) + 8 * o, 8 * n, hipMemcpyHostToDevice, s));
        OV2_HIP_CHECK(hipMemcpyAsync(t->depi + L0.o_kb + 24 * o, kh + (L0.o_kb - L0.o_kl) + 24 * o, 24 * n, hipMemcpyHostToDevice, s));
    }
    t->kf_hdr[(size_t)item] = h;
    OV2_HIP_CHECK(hipMemcpyAsync(t->dfx + sizeof(FeKfHdr) * (size_t)item, &t->kf_hdr[(size_t)item], sizeof(FeKfHdr), hipMemcpyHostToDevice, s));
    OV2_HIP_CHECK(hipStreamSynchronize(s));                              // the host copy may be rewritten by the next call
    return OV2_OK;
}

int ov2_btracker_track_frame_epi_pose_begin(ov2_btracker *t, int n_active, const uint8_t *const *img_h, int stride, const float *kps_xy_h,
                                            const double *wpt_h, const uint8_t *is3d_h, const double *Tcw_h, const int *n_h,
                                            int klt_use_prior, const ov2_frame_epi_pose_params *params,
                                            const ov2_frame_epi_pose_input *input)
{
    return track_frame_begin(t, n_active, img_h, stride, kps_xy_h, nullptr, nullptr, n_h, klt_use_prior, true, wpt_h, is3d_h, Tcw_h,
                             true, nullptr, nullptr, true, params, input);
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
    if (t && n_active >= 1 && n_active <= t->batch && n_h) {              // as ov2_btracker_track_frame: the result buffers before anything is enqueued
        int n_total = 0;
        for (int b = 0; b < n_active; b++) {
            n_total += n_h[b] > 0 ? n_h[b] : 0;
            OV2_REQUIRE(n_h[b] <= 0 || (pose_results[b].removed && epi_results[b].removed), OV2_EINVAL, "NULL result buffer (removed)");
            OV2_REQUIRE(!epi_results[b].trace_samples, OV2_EINVAL, "trace_samples must be NULL in a step: ov2_btracker_last_epi_inputs fetches the table");
        }
        OV2_REQUIRE(n_total == 0 || (out_xy_h && status_h), OV2_EINVAL, "NULL point buffer");
    }
    const int rc = ov2_btracker_track_frame_epi_pose_begin(t, n_active, img_h, stride, kps_xy_h, wpt_h, is3d_h, Tcw_h, n_h, klt_use_prior, params, input);
    if (rc != OV2_OK) return rc;
    return track_frame_end(t, out_xy_h, status_h, p3p_req, pose_results, epi_results);
}

int ov2_btracker_last_epi_inputs(const ov2_btracker *t, int item, int *n_cur, int *slot_idx, int *m, int *samples, int *n_rows_used)
{
    OV2_REQUIRE(t, OV2_EINVAL, "NULL tracker");
    OV2_REQUIRE(item >= 0 && item < t->batch, OV2_EINVAL, "batch item out of range");
    OV2_REQUIRE(t->le_on, OV2_EINVAL, "ov2_btracker_last_epi_inputs: no epipolar step has been finished on this tracker");
    const size_t b = (size_t)item;
    const int nc = t->le_ncur[b], rows = t->le_rows[b];
    if (n_cur) *n_cur = nc;
    if (m) *m = t->le_m[b];
    if (n_rows_used) *n_rows_used = rows;
    if (t->le_host[b]) {
        if (slot_idx && nc > 0) memcpy(slot_idx, t->le_slot[b].data(), 4 * (size_t)nc);
        if (samples && rows > 0) memcpy(samples, t->le_samples[b].data(), 32 * (size_t)rows);
        return OV2_OK;
    }
    if (!t->le_chain || (nc <= 0 && rows <= 0)) return OV2_OK;
    OV2_HIP_CHECK(hipSetDevice(t->ctx->device));
    const EpifLayout &L = t->le_L;
    const size_t nm = (size_t)t->cfg.n_max;
    if (slot_idx && nc > 0 && (size_t)nc <= nm)
        OV2_HIP_CHECK(hipMemcpy(slot_idx, t->dfx + t->x_slot + 4 * b * nm, 4 * (size_t)nc, hipMemcpyDeviceToHost));
    if (samples && rows > 0)
        OV2_HIP_CHECK(hipMemcpy(samples, t->depi + L.o_sm + 32 * b * (size_t)L.s_max, 32 * (size_t)rows, hipMemcpyDeviceToHost));
    return OV2_OK;
}

int ov2_btracker_track_frame(ov2_btracker *t, int n_active, const uint8_t *const *img_h, int stride, const float *kps_xy_h,
                             const float *prior_xy_h, const uint8_t *has_prior_h, const int *n_h, int klt_use_prior,
                             float *out_xy_h, uint8_t *status_h, int *p3p_req)
{
    if (t && n_active >= 1 && n_active <= t->batch && n_h) {              // (the one-call form checks its result buffers before anything is enqueued)
        int n_total = 0;
        for (int b = 0; b < n_active; b++) n_total += n_h[b] > 0 ? n_h[b] : 0;
        OV2_REQUIRE(n_total == 0 || (out_xy_h && status_h), OV2_EINVAL, "NULL point buffer");
    }
    const int rc = ov2_btracker_track_frame_begin(t, n_active, img_h, stride, kps_xy_h, prior_xy_h, has_prior_h, n_h, klt_use_prior);
    if (rc != OV2_OK) return rc;
    return ov2_btracker_track_frame_end(t, out_xy_h, status_h, p3p_req);
}

int ov2_btracker_track_frame_map(ov2_btracker *t, int n_active, const uint8_t *const *img_h, int stride, const float *kps_xy_h,
                                 const double *wpt_h, const uint8_t *is3d_h, const double *Tcw_h, const int *n_h, int klt_use_prior,
                                 float *out_xy_h, uint8_t *status_h, int *p3p_req)
{
    if (t && n_active >= 1 && n_active <= t->batch && n_h) {              // as ov2_btracker_track_frame: the result buffers before anything is enqueued
        int n_total = 0;
        for (int b = 0; b < n_active; b++) n_total += n_h[b] > 0 ? n_h[b] : 0;
        OV2_REQUIRE(n_total == 0 || (out_xy_h && status_h), OV2_EINVAL, "NULL point buffer");
    }
    const int rc = ov2_btracker_track_frame_map_begin(t, n_active, img_h, stride, kps_xy_h, wpt_h, is3d_h, Tcw_h, n_h, klt_use_prior);
    if (rc != OV2_OK) return rc;
    return ov2_btracker_track_frame_end(t, out_xy_h, status_h, p3p_req);
}

int ov2_btracker_last_priors(const ov2_btracker *t, int item, int n, float *prior_xy_h, uint8_t *has_prior_h)
{
    OV2_REQUIRE(t, OV2_EINVAL, "NULL tracker");
    OV2_REQUIRE(item >= 0 && item < t->batch, OV2_EINVAL, "batch item out of range");
    OV2_REQUIRE(n >= 0 && n <= t->last_pn[(size_t)item], OV2_EINVAL, "more keypoints than the last tracking call returned for this item");
    const size_t o = (size_t)item * t->cfg.n_max;
    if (prior_xy_h) memcpy(prior_xy_h, t->hblk + t->o_pri + 8 * o, 8 * (size_t)n);
    if (has_prior_h) memcpy(has_prior_h, t->hblk + t->o_flg + o, (size_t)n);
    return OV2_OK;
}

int ov2_btracker_last_keypoints(const ov2_btracker *t, int item, int n, float *unpx_xy_h, double *bv_xyz_h)
{
    OV2_REQUIRE(t && t->has_calib, OV2_EINVAL, "no calibration set on this tracker");
    OV2_REQUIRE(item >= 0 && item < t->batch, OV2_EINVAL, "batch item out of range");
    OV2_REQUIRE(n >= 0 && n <= t->last_n[(size_t)item], OV2_EINVAL, "more keypoints than the last tracking call returned for this item");
    const size_t o = (size_t)item * t->cfg.n_max;
    if (unpx_xy_h) memcpy(unpx_xy_h, t->hblk + t->o_unpx + 8 * o, 8 * (size_t)n);
    if (bv_xyz_h) memcpy(bv_xyz_h, t->hblk + t->o_bv + 24 * o, 24 * (size_t)n);
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
