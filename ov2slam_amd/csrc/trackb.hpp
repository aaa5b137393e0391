// trackb.hpp -- what the translation units of the lock-step tracker share (trackb.hip: the tracker, its steps, the resident state;
// trackb_keyframe.hip: the keyframe calls): the block types, struct ov2_btracker and the helpers both use.  Declarations only: the
// definitions are trackb.hip's.
#pragma once
#include "common.hpp"
#include "keypoint_dev.hpp"
#include "pose_dev.hpp"
#include "frameepi_dev.hpp"
#include "mono_dev.hpp"
#include "detect_dev.hpp"
#include "createkf_dev.hpp"
#include "resident_dev.hpp"
#include "stereokf_dev.hpp"
#include "temporalkf_dev.hpp"
#include "mvg_dev.hpp"
#include "fkf_dev.hpp"
#include "kltkf_dev.hpp"
#include "monoinit_dev.hpp"
#include "trackb_layout.hpp"
#include <deque>
#include <initializer_list>
#include <vector>

#define BT_SETS 8       // pyramid sets in rotation: cur, prev, the one being prepared for the next frame, five of slack for the mapper
                        // context (a keyframe's pyramids outlive it by BT_SETS - 1 steps: the keyframe period of the shipped parameter files)
#define BT_IMG_SETS 3   // staging sets: frame f (read by its pre-processing), f + 1 (arriving), f + 2 (being filled by the host)

// A block the host fills and reads and the kernels read and write: pinned + mapped, reached by the kernels through its device alias
// (zero copy), or mirrored on the device with a copy up before the kernels and a copy down behind them.
struct IoBlock {
    uint8_t *h = nullptr, *d = nullptr, *k = nullptr;    // the pinned block; its device mirror (NULL with zero copy); what the kernels dereference
    size_t bytes = 0;
    // decide: the tracker's first block takes the alias when there is one and sets zero_copy; the later blocks follow it
    int alloc(size_t n, bool &zero_copy, bool decide, const char *who);
    void release();
    // [0, n) up, [from, to) down: nothing to do when the kernels work on the pinned block itself
    int upload(hipStream_t s, size_t n) const { return upload(s, 0, n); }
    int upload(hipStream_t s, size_t from, size_t to) const;
    int download(hipStream_t s, size_t from, size_t to) const;
};

// A block of the calls around the step: a device allocation, zero-filled on the stream before its first use, and optionally a pinned
// host block over its first host_bytes (the device-only work ranges lie behind the part that travels).  ALWAYS mirrored with explicit
// copies: the kernels never read these over the zero-copy alias of IoBlock.  (Not common.hpp's Stage either: that lives in the
// context's scratch, which other calls reuse on the same stream between a _begin and its _end.)
struct DevBlock {
    uint8_t *h = nullptr, *d = nullptr;
    size_t dev_bytes = 0;
    // on any failure: what was taken is freed, the sticky error cleared, the error text "<who>: <hip error string>", OV2_ENOMEM
    int alloc(size_t host_bytes, size_t n, hipStream_t s, const char *who);
    // the device half anew at `need` zeroed bytes (the host half stays): for the grow-only blocks, whose callers compare the sizes
    int grow(size_t need, hipStream_t s, const char *who);
    void release();
    int up(hipStream_t s, size_t from, size_t to) const;                // [from, to) of the pinned half to the same place on the device
    int down(hipStream_t s, size_t from, size_t to) const;              // and back
    int fail(hipError_t e, const char *who);
};

// all of the blocks or none: the allocations in order; when one fails, every block of the list is released again
struct DevBlockSpec { DevBlock *b; size_t host_bytes, dev_bytes; };
int alloc_all(std::initializer_list<DevBlockSpec> blocks, hipStream_t s, const char *who);

// the forms of a step (trackb.hip: StepArgs); each includes the one before it, STEP_MONO resolves to POSE or EPI plus Pending::mono
enum StepForm { STEP_PLAIN = 0, STEP_MAP, STEP_POSE, STEP_EPI, STEP_MONO };

// ov2_btracker_last_pose_inputs / ov2_btracker_last_epi_inputs: what the last finished step of the kind fed its chain.  Per item the
// counts (ncur: entries of the slot list -- the filter's packed frame; the pose set, so m again) and, for an item the 33 % rule
// re-ran (host), the slot list and the table of the second run -- the device block still holds those of the first
struct LastInputs {
    bool on = false, chain = false;                  // a step has been finished; its chain ran (not a first frame / nothing tracked)
    std::vector<int> ncur, m, rows;
    std::vector<std::vector<int>> slot, samples;
    std::vector<uint8_t> host;
    void open(size_t B, bool tracked)
    {
        on = true; chain = tracked;
        ncur.assign(B, 0); m.assign(B, 0); rows.assign(B, 0); host.assign(B, 0); slot.resize(B); samples.resize(B);
    }
};

// the calls that stay open between a _begin and its _end
enum OpenCall { CALL_NONE = 0, CALL_STEP, CALL_CKF, CALL_SKF, CALL_TKF, CALL_MINIT };

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
    size_t img_pitch = 0, img_bytes = 0;          // per item (trackb_layout.hpp)
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
    // the four blocks the host and the kernels share (IoBlock; their sections: trackb_layout.hpp).  The point block decides zero_copy
    // for all of them; the map, pose and epipolar blocks are allocated by the first step of their form
    IoBlock pt, map, pose, epi, mono;
    bool zero_copy = false;
    BtPointLayout pl; BtMapLayout ml; BtPoseLayout ql; BtEpiLayout el; BtMonoLayout nl;
    // ov2_btracker_track_mono: the resident block (frame pose, motion state, keyframe info per item) with its host mirrors, and the
    // work block of k_mono_pack / k_fkf_parallax (both device only), allocated by the first setter or step of the kind
    DevBlock res, mw;
    std::vector<double> res_T, res_kt;
    std::vector<ov2_motion_state> res_st;
    std::vector<MonoKfInfo> res_ki;
    bool has_calib = false;
    KpCalib calib;
    std::vector<int> last_n;           // per item: keypoints of the last track_frame (0 before / after a call that tracked nothing)
    std::vector<int> last_pn;          // the same whether or not a calibration is set (ov2_btracker_last_priors)
    // ov2_btracker_track_frame_pose: the chain's block at capacity and the pack's lists (device only, grow-only; not the context's
    // scratch, which other calls use on the same stream)
    DevBlock work;
    LastInputs lp;
    PoseLayout lp_L;                                  // the chain's layout in the last finished pose step
    // ov2_btracker_track_frame_epi_pose / ov2_btracker_set_keyframe: the epipolar side, allocated by the first of either.
    //   depi   the filter's block (EpifLayout at capacity: batch x n_max slots, batch x n_rows rows; device only, grow-only).  Its
    //          inputs [0, o_up) do not depend on n_rows, so the resident keyframe arrays stay where they are when a step asks for
    //          more rows and the block is grown (they are then copied again from kf_host).
    //          A raw pointer, not a DevBlock: the grown block is seeded from kf_host BEFORE the old one is freed (ensure_epi).
    //   fx     the index block (device only)
    uint8_t *depi = nullptr;
    size_t depi_bytes = 0;
    DevBlock fx;
    EpifLayout eL0;                                   // the layout with no rows: where the keyframe arrays lie
    std::vector<uint8_t> kf_host;                     // host copy of the block's [o_kl, o_up)
    std::vector<FeKfHdr> kf_hdr;
    FeStep fe;                                        // the arguments of the step being enqueued
    LastInputs le;
    EpifLayout le_L;                                  // the filter's layout in the last finished epipolar step
    // keyframe detection: device mirrors of the items' current keypoints and of the detector's output, pinned staging
    DevBlock det, out; int out_cap = 0;
    DevBlock roi;                                 // detectGFTT: device copy of the caller's roi mask (w x h, allocated with the first one)
    // a step between ov2_btracker_track_frame_begin and _end: what _end needs to finish it
    struct Pending { bool tracked = false; StepForm form = STEP_PLAIN; int n_active = 0, use_prior = 0;
                     const float *kps = nullptr; const uint8_t *has_prior = nullptr; std::vector<int> n;
                     // pose and epi: the settings and the per-item inputs _end needs again (the filter's per-item inputs stay in the
                     // epipolar block, which the device only reads)
                     ov2_frame_pose_params pp; PoseLayout L; std::vector<double> Twc; std::vector<uint8_t> req;
                     std::vector<unsigned long long> seed;
                     ov2_epifilter_params ep; EpifLayout eL;
                     // mono: the step runs between the motion model and the decision; ran: not the tracker's first frame
                     bool mono = false, mono_ran = false; ov2_fkf_params fkf; std::vector<double> time;
                     std::vector<int> frame_id, localba;
                     bool resident = false;               // the frame is the resident one; k_res_carry wrote the next one
                     bool from_kf = false; } pend;        // the step tracked from the keyframe store (kltTrackingFromKF)
    // the raw frames of the current step: items [0, raw_n) of dimg[raw_which], until that set is uploaded / prepared again (describeBRIEF)
    int raw_which = -1, raw_n = 0;
    // ov2_btracker_create_keyframe, allocated by its first call: the I/O block (pinned, and its device mirror at the same offsets:
    // BtCkfLayout) and the detector's work block (device only, grow-only: the output lists, then one pass's maps, candidates and
    // free-cell lists)
    BtCkfLayout cl;
    DevBlock ckf, ckw;
    struct CkfPending { bool det = false; int n_active = 0, mode = 0, ncells = 0; ov2_create_keyframe_params p;
                        double *quality = nullptr; int *fast_th = nullptr; std::vector<uint8_t> flag; std::vector<int> nkfid;
                        std::vector<double> time; bool resident = false, from_kf = false; } cpend;
    // the resident frame (f21), allocated by its first use: the frame block (two buffers of `batch` items: BtResLayout) with its
    // pinned host mirror of the same layout, the control block of a call (pinned, and its device mirror), and per item the buffer
    // that holds the current frame
    BtResLayout rl;
    DevBlock fr, ctl;
    std::vector<uint8_t> res_sel;
    size_t slot_bytes = 0;            // ov2_btracker_last_slot_bytes
    // ov2_btracker_stereo_keyframe (f22), allocated by its first call: the I/O block (pinned [0, s_down), and its device mirror with the
    // work ranges behind: BtSkfLayout, regrown when a call's grid has more cells), per item whether its resident frame is its resident
    // keyframe, and the call between _begin and _end
    BtSkfLayout sl;
    int skf_cells = -1;
    DevBlock skf;
    std::vector<uint8_t> res_iskf;
    struct SkfPending { int n_active = 0; std::vector<uint8_t> action; } spend;
    // ov2_btracker_temporal_keyframe (f23), allocated by the first call that needs it: the anchor block (two buffers, item-major) and
    // its pinned mirror, per item the buffer of its current table, the call's I/O block (pinned [0, t_down), and its device mirror with
    // the work ranges behind), the block of ov2_btracker_set_anchor_poses, and the call between _begin and _end
    BtTkfLayout tl;
    int n_src_max = 0;
    DevBlock anc, tkf, ap;
    std::vector<uint8_t> anc_sel;
    struct TkfPending { int n_active = 0; std::vector<uint8_t> action; } tpend;
    // the from-keyframe mode (ov2_btracker_set_track_from_keyframe; kltkf.hip), allocated by its first `on`: the keyframe store -- one
    // more pyramid set of `batch` items outside the rotation, with its item views -- the keyframe-px table with its pinned mirror
    // (BtKfPxLayout), and per item whether a pyramid has been adopted
    bool from_kf = false;
    ov2_pyr *kf_store = nullptr;
    std::vector<ov2_pyr *> kf_view;
    BtKfPxLayout kl;
    DevBlock kfpx;
    std::vector<uint8_t> kf_has_pyr;
    // ov2_btracker_mono_init (f25), allocated by its first call: the I/O block (pinned [0, i_down), and its device mirror with the
    // chain's block behind: BtMinitLayout, regrown when a call draws more rows), and the call between _begin and _end
    BtMinitLayout il;
    int mi_rows = -1;
    DevBlock mi;
    struct MinitPending { int n_active = 0; std::vector<uint8_t> action; } ipend;
    // the call between a _begin and its _end: at most one at a time (begin_guard)
    OpenCall open = CALL_NONE;
    bool open_call() const { return open != CALL_NONE; }
};

// ---- the helpers both translation units use (trackb.hip) ----
int begin_guard(const ov2_btracker *t, OpenCall who);             // what the _begin of a call of kind `who` refuses: any open call
int ensure_epi(ov2_btracker *t, const EpifLayout *L);            // the epipolar side's buffers; the filter's block grown to layout L (or NULL)
int ensure_mono(ov2_btracker *t);                                // the mono side's buffers, the resident block with its host mirrors
int ensure_res(ov2_btracker *t);                                 // the resident frame's blocks: every frame empty
int mono_item(ov2_btracker *t, int item, const char *open_msg);  // the item, no open call, ensure_mono
// item b of the resident frame's host mirror: its current frame (other == 0) or the buffer its next frame is written into (other == 1)
struct ResHost { int *n; float *px; int *lmid; uint8_t *is3d; double *wpt; };
ResHost res_host(const ov2_btracker *t, int b, int other);
ResFrames res_frames(const ov2_btracker *t);
int res_push_sel(ov2_btracker *t, hipStream_t s);                // which buffer holds each item's current frame, to the device
// item b's keyframe arrays in kf_host (the block's [o_kl, o_up) as the layout without rows puts them)
struct KfHost { int *lmid; float *unpx; double *bv; };
KfHost kf_host_item(ov2_btracker *t, int b);
KfPxTable kfpx_table(const ov2_btracker *t);                     // the device view of the keyframe-px table
