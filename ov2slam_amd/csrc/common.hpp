// common.hpp -- shared declarations of libov2slam_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include <stdio.h>
#include <string.h>
#include <string>
#include <vector>
#include "../../include/ov2slam_hip.h"
#include "stage.hpp"

#define OV2_MAX_LEVELS 8

// ---- error plumbing (never throws across the C ABI) ------------------------
void ov2_set_error(const char *fmt, ...);

#define OV2_HIP_CHECK(expr)                                                        \
    do {                                                                           \
        hipError_t _e = (expr);                                                    \
        if (_e != hipSuccess) {                                                    \
            ov2_set_error("%s:%d: %s -> %s", __FILE__, __LINE__, #expr,            \
                          hipGetErrorString(_e));                                  \
            return OV2_EHIP;                                                       \
        }                                                                          \
    } while (0)

#define OV2_REQUIRE(cond, code, msg)                                               \
    do {                                                                           \
        if (!(cond)) {                                                             \
            ov2_set_error("%s:%d: %s", __FILE__, __LINE__, msg);                   \
            return (code);                                                         \
        }                                                                          \
    } while (0)

// ---- context ---------------------------------------------------------------
struct ov2_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool owns_stream = false;
    // grow-only scratch (device + pinned host), reused across calls of this ctx
    void *d_scratch = nullptr;  size_t d_scratch_bytes = 0;
    void *h_scratch = nullptr;  size_t h_scratch_bytes = 0;
    // LK statistics: work-groups add their (iterations, patch builds) into one of LK_STAT_SLOTS cache lines
    // (same-address device atomics retire at ~6 ns each: 2 per work-group on one address would put a
    // 200 us floor under a 16k-work-group launch); a one-block kernel folds the lines into the caller's pair.
    unsigned long long *stat_slots = nullptr;
    // persistent k_fb_klt3 (lk3.hip): pull counters, list lengths and unit lists of one launch (lk_plan.hpp; grow-only, re-made by every
    // launch on the stream) and the number of work-groups the device holds at once (0: not queried yet)
    int *lk_plan = nullptr;  size_t lk_plan_ints = 0;
    int lk_resident_wgs = 0;
    int sobel_dy_order = OV2_SOBEL_DY_OPENCV_ROWFILTER;   // ov2_ctx_set_option(OV2_OPT_SOBEL_DY_ORDER)
    // Path selection / test forcing (ov2_ctx_set_option, OV2_OPT_*).  The library reads NO environment variable after
    // ov2_ctx_create: the entry points are called from several threads of a host that may setenv() concurrently.
    int lk_impl = OV2_LK_IMPL_AUTO;            // OV2_OPT_LK_IMPL
    int lk_persist = -1;                       // OV2_OPT_LK_PERSIST: -1 auto, 0 one work-group per keypoint block, N > 0 persistent with N work-groups
    int track_impl = OV2_TRACK_IMPL_WAVE;      // OV2_OPT_TRACK_IMPL
    int lk_acc = OV2_LK_ACC_INT64;             // OV2_OPT_LK_ACC
    int clahe_strips = -1;                     // OV2_OPT_CLAHE_STRIPS: -1 auto, 0 never, 1 whenever the geometry allows
    int ba_force_large = 0;                    // OV2_OPT_BA_FORCE_LARGE
    int ba_lin_direct = 0;                     // OV2_OPT_BA_LIN_DIRECT
    int ba_schur_chunk = 0;                    // OV2_OPT_BA_SCHUR_CHUNK (columns; 0 = auto)
    int ba_xyz_lin_waves = 0;                  // OV2_OPT_BA_XYZ_LIN_WAVES (0 = auto, 1, 2)
    int ba_pose_only_fused = 1;                // OV2_OPT_BA_POSE_ONLY_FUSED
    int ba_deterministic = 0;                  // OV2_OPT_BA_DETERMINISTIC
    int ba_trace = 0;                          // OV2_OPT_BA_TRACE: the one-problem solves record their iteration summaries (ov2_ba_get_trace)
    void *ba_trace_d = nullptr, *ba_trace_h = nullptr; int ba_trace_n = 0;
    int det_fast_tie = 1;                      // OV2_OPT_FAST_TIE: OV2_FAST_TIE_LIBSTDCXX (the reference as built with g++)
    hipStream_t det_aux_stream = nullptr; hipEvent_t det_ev[2] = {nullptr, nullptr};   // batched detectors: the passes alternate between the context's stream and this one
    int det_strip = -1;                        // OV2_OPT_DETECT_STRIP: -1 auto (batches), 0 one wavefront per cell, 1 the strip kernel
    // BRIEF test pairs (ov2_brief_set_pattern): the caller's table when brief_custom, the built-in one otherwise; the 1 KB device copy
    // is (re)uploaded on the stream before the next describe call after a change
    int8_t brief_pat[256 * 4] = {};  bool brief_custom = false;
    void *brief_pat_d = nullptr;  bool brief_pat_current = false;
    void *ba_det_pool = nullptr; size_t ba_det_bytes = 0;   // OV2_OPT_BA_DETERMINISTIC: per-work-group copies of H / F^T b / G (grow-only)
    // ov2_local_ba_batch: persistent host threads that prepare the problems of a batch (created with the first batch; ba.hip owns the type)
    void *ba_host_pool = nullptr; void (*ba_host_pool_free)(void *) = nullptr;
    hipEvent_t ba_ev[2] = {nullptr, nullptr};              // the two timing events of a solve (created with the first one: a pair per pass was 25 us)
    int lckf_scratch_kb = 256 * 1024;          // OV2_OPT_LCKF_SCRATCH_KB: device scratch one chunk of ov2_lckf_prepare* items may take
    int epif_capacity = 0;                     // OV2_OPT_EPIF_CAPACITY: ov2_epipolar_filter_batch stages its block in the capacity form
    int debug = 0;                             // OV2_OPT_DEBUG; initial value: environment OV2_DEBUG, read once by ov2_ctx_create
    // pinned staging of host images on their way to the device: its own buffer (h_scratch is rewritten by the next call's small
    // arrays while an asynchronous image upload may still be in flight) and an event that says when it may be refilled
    void *h_img = nullptr;  size_t h_img_bytes = 0;
    hipEvent_t img_ev = nullptr;  bool img_pending = false;
    int reserve_device(size_t bytes);
    int reserve_host(size_t bytes);
    int reserve_stat_slots();
    int reserve_lk_plan(size_t ints);
    // host image (any row stride, pageable or pinned) -> device buffer with pitch dst_pitch, asynchronous on the stream; the
    // caller's buffer is free again when this returns
    int upload_image(void *dst_d, size_t dst_pitch, const uint8_t *src_h, size_t src_stride, size_t w, size_t h);
    // n images (one pointer each) into device slots `item_bytes` apart: one repack into the pinned staging buffer, ONE DMA
    int upload_images(void *dst_d, size_t dst_pitch, size_t item_bytes, const uint8_t *const *src_h, int n, size_t src_stride, size_t w, size_t h);
    // the reverse, synchronous: h rows of w bytes at device pitch src_pitch -> host rows at dst_stride (one contiguous DMA into the
    // pinned staging buffer, then a host-side repack)
    int download_image(uint8_t *dst_h, size_t dst_stride, const void *src_d, size_t src_pitch, size_t w, size_t h);
};
// The round trip of a stand-alone call (host conventions), after its input checks: ONE scratch block whose sections
// (StageCursor, stage.hpp) lie at the same offsets on the device (d) and in the pinned host block (h).  open() sets the device and
// reserves both grow-only scratches (a block may be shorter on the host: only what travels needs room there); the caller packs the
// inputs into h, uploads, launches on ctx->stream, downloads, syncs once and scatters from h.  Every step returns an OV2_* code.
struct Stage {
    ov2_ctx *ctx = nullptr;
    uint8_t *h = nullptr, *d = nullptr;
    int open(ov2_ctx *ctx, size_t dev_bytes, size_t host_bytes);
    // device [begin, end) from the same host offsets
    int upload(size_t begin, size_t end) const { OV2_HIP_CHECK(hipMemcpyAsync(d + begin, h + begin, end - begin, hipMemcpyHostToDevice, ctx->stream)); return OV2_OK; }
    // device [begin, end) to host offset `at`
    int download(size_t begin, size_t end, size_t at) const { OV2_HIP_CHECK(hipMemcpyAsync(h + at, d + begin, end - begin, hipMemcpyDeviceToHost, ctx->stream)); return OV2_OK; }
    int sync() const { OV2_HIP_CHECK(hipStreamSynchronize(ctx->stream)); return OV2_OK; }
};
#define LK_STAT_SLOTS 256
#define LK_STAT_STRIDE 16      // unsigned long long per slot (128 B)

// ---- pyramid layout in HBM ---------------------------------------------------
// One allocation per ov2_pyr holding `batch` items of identical layout.  Per
// level: a padded u8 image (REFLECT_101 border, ROI origin 16-byte aligned) and a
// padded int16x2 Scharr derivative (zero border, ROI origin 64-byte aligned).
struct PyrLevelDesc {
    int w, h;
    int img_pitch;        // bytes per padded image row (multiple of 64)
    int der_pitch;        // int16x2 elements (4 B) per padded derivative row (multiple of 16)
    long long img_roi;    // byte offset (from the item base) of image ROI pixel (0,0)
    long long der_roi;    // byte offset (from the item base) of derivative ROI element (0,0)
    int img_padx, der_padx, pady;
};

struct PyrDesc {
    uint8_t *base;            // device pointer of batch item 0
    long long item_stride;    // bytes between batch items
    int n_levels;
    int win;
    int batch;
    PyrLevelDesc lv[OV2_MAX_LEVELS];
};

struct ov2_pyr {
    PyrDesc d;
    int w = 0, h = 0, max_level = 0;
    size_t bytes = 0;
    int device = 0;
    // Cross-context hand-off (the front-end's pyramid is read by the mapper thread's context):
    // every (re)build records `ready` on the producing stream; a consumer entry point running on another stream
    // waits on it before its first kernel (ov2_pyr_wait_ready).  Same-stream use costs nothing.
    hipEvent_t ready = nullptr;
    hipStream_t producer = nullptr;
    bool built = false;
    // ov2_pyr_item_view: a batch-1 alias of one item of `parent` (owns neither the memory nor the event; the hand-off state is the parent's)
    const ov2_pyr *parent = nullptr;
};
int ov2_pyr_mark_ready(ov2_ctx *ctx, ov2_pyr *p);              // after the last kernel of a build was enqueued
int ov2_pyr_wait_ready(ov2_ctx *ctx, const ov2_pyr *p);        // before the first kernel of a consumer

// ---- rectification map (rectify.hip) -----------------------------------------
// Both map forms of ov2_rectmap_create normalised to one device representation; immutable after creation.
struct ov2_rectmap {
    int device = 0, w = 0, h = 0;
    int pitch = 0;              // map entries per row: w rounded up to 4 (the kernel's vector loads stay aligned)
    uint32_t *ixy = nullptr;    // (uint16)ix | (uint16)iy << 16
    uint16_t *ab = nullptr;     // b * 32 + a
};

// kernels' host launchers (defined in the .hip files)
// cv::remap (INTER_LINEAR, BORDER_CONSTANT 0) of n_items device images through `m` (k_remap): src and dst must not overlap
int ov2_launch_remap(hipStream_t stream, const ov2_rectmap *m, const uint8_t *src_d, size_t src_pitch, size_t src_item, int n_items,
                     uint8_t *dst_d, size_t dst_pitch, size_t dst_item);
// from_level = 1: levels 0 and 1 (borders included) are already in place (k_clahe_apply_pyr)
int ov2_launch_pyr_build(ov2_ctx *ctx, ov2_pyr *p, const uint8_t *img_d, int stride, size_t img_batch_stride, int from_level = 0);
// cv::CLAHE::apply on `batch` device images; border > 0: dst is a padded pyramid level, its REFLECT_101 border is written too
int ov2_launch_clahe(ov2_ctx *ctx, const uint8_t *src_d, int w, int h, int stride, size_t src_batch_stride, int batch,
                     double clip_limit, int tiles_x, int tiles_y, uint8_t *dst_d, int dst_stride, size_t dst_batch_stride,
                     uint8_t *lut_d, int border, const struct PyrDesc *pyr = nullptr, int *level1_done = nullptr);
// fused VisualFrontEnd::kltTracking launch (lk.hip), device pointers only
int ov2_launch_track_klt(hipStream_t s, const ov2_pyr *prev, const ov2_pyr *cur, int win, int lvl_prior, int lvl_full,
                         int max_iter, float eps, float err_th, float fb_dist, int n_max, const int *n_dev,
                         const float *kps, const float *priors, const uint8_t *flags, float *out_xy, uint8_t *status, int *iters,
                         const float *sad_x = nullptr, float sad_up = 0.f,       // sad_x: stereo mode (lk.hip: k_track_klt)
                         int track_impl = OV2_TRACK_IMPL_WAVE,
                         int items = 1,    // items > 1 (trackb.hip): batch items [0, items) of both pyramids, n_max point slots and one n_dev entry per item
                         int lk_acc = OV2_LK_ACC_INT64);   // OV2_OPT_LK_ACC   // items > 1 (trackb.hip): batch items [0, items) of both pyramids, n_max point slots and one n_dev entry per item
// fused VisualFrontEnd::kltTrackingFromKF launch (lk.hip): kf is the keyframe's pyramid, kps the keyframe's px, a lost prior track is
// retried from retry_prior, flag bit 1 skips a slot (status 4); the kernel choice is ov2_launch_track_klt's
int ov2_launch_track_klt_kf(hipStream_t s, const ov2_pyr *kf, const ov2_pyr *cur, int win, int lvl_prior, int lvl_full,
                            int max_iter, float eps, float err_th, float fb_dist, int n_max, const int *n_dev,
                            const float *kps, const float *priors, const float *retry_prior, const uint8_t *flags, float *out_xy,
                            uint8_t *status, int *iters, int track_impl = OV2_TRACK_IMPL_WAVE, int items = 1, int lk_acc = OV2_LK_ACC_INT64);
// The cross-keypoint rule of visual_front_end.cpp:225-230 over the n results of one frame (track.hip; both trackers call it): when
// fewer than 33 % of the prior tracks are good, the lost ones are run again from their keypoints between the two pyramids (one item
// each), out_xy / status take the new results and *p3p_req (may be NULL) is set.  calib != NULL: unpx (2 per keypoint) and bv (3 per
// keypoint) of the re-run keypoints follow their new positions.
struct KpCalib;
struct P3pRuleFrame { const float *kps; const uint8_t *has_prior; int use_prior, n; float *out_xy; uint8_t *status; float *unpx; double *bv; };
int ov2_apply_p3p_rule(ov2_ctx *ctx, const ov2_tracker_config &cfg, const ov2_pyr *prev, const ov2_pyr *cur, const KpCalib *calib,
                       const P3pRuleFrame &f, int *p3p_req);

// BRIEF descriptors (brief.hip) of the points of items [0, n_items) of a device image batch (items item_stride bytes apart), from host
// point arrays with cap slots per item (n_h[b] valid; NULL: n_h_all each) into host outputs of the same layout (slots past n_h[b]
// untouched).  img_h != NULL: a host image of one item, uploaded to the context's scratch first (img_d is ignored).  ONE host
// synchronisation; the kernel is enqueued on ctx->stream after everything already there (so after the frame's H2D of a tracker).
int ov2_brief_run_h(ov2_ctx *ctx, const uint8_t *img_h, const uint8_t *img_d, int w, int h, size_t pitch, size_t item_stride, int n_items,
                    const float *xy_h, const int *n_h, int n_h_all, int cap, uint8_t *desc_h, uint8_t *valid_h);

// k_brief32 on device points, enqueued on ctx->stream with no synchronisation (the context's pattern: uploaded first when it changed):
// n_items images item_stride apart, cap point slots per item, n_d[b] of them live (NULL: n_all each)
int ov2_brief_launch_d(ov2_ctx *ctx, const uint8_t *img_d, int w, int h, size_t pitch, size_t item_stride, int n_items,
                       const float *xy_d, int cap, const int *n_d, int n_all, uint8_t *desc_d, uint8_t *valid_d);

// the loop closer's keyframe preparation (lckf.hip) on items [0, n_items) of a device image batch, or on one host image (img_h != NULL:
// uploaded to the context's scratch first, img_d is ignored): host exclusion points with excl_cap slots per item, one result per item.
// ONE upload, ONE download, ONE host synchronisation; the inputs are checked before the context is touched.
int ov2_lckf_run_h(ov2_ctx *ctx, const uint8_t *img_h, const uint8_t *img_d, int w, int h, size_t pitch, size_t item_stride, int n_items,
                   const ov2_lckf_params *params, const float *excl_xy_h, const int *n_excl_h, int excl_cap, ov2_lckf_result *results);

// cv::cornerSubPix (detect.hip, k_corner_subpix) on device points, one wavefront per point slot: `items` images img_item_stride bytes
// apart, n slots per item xy_item_stride points apart; n_dev (ints ndev_item_stride apart) holds each item's live count on the
// device (NULL: n).  Asynchronous on `stream`; used by the detectors of detect.hip and gftt.hip.
int launch_subpix(hipStream_t stream, const uint8_t *img_d, int w, int h, int stride, float2 *xy_d, int n,
                  int half_win, int max_iter, double eps, const int *n_dev = nullptr,
                  int items = 1, long long img_item_stride = 0, int xy_item_stride = 0, int ndev_item_stride = 0);
